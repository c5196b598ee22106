"""The counting form of the confidence maps (csrc/confidence_stats.hip) on small maps, integer for integer: the histograms of
xv_confidence_stats and xv_fused_head_multi_confidence_stats_fwd must equal uncertainty_model.confidence_tables_reference --
bin_index on the host -- of the maps ops.confidence_map / ops.fused_head_multi_confidence write for the same inputs, the class
counts must be exact, and the NLL sums are compared with the nll column of ops.calibration_table /
ops.fused_head_multi_calibration at the same temperature.

The NLL bound.  Both sides add the SAME float32 terms (calib_pixel) as doubles, but in another order: here per class into LDS
copies, there per temperature into 32 copies.  A double sum of n <= 2^15 non-negative terms carries at most n 2^-53 relative
error whatever the order, 2^-38 < 1e-11; the issue allows 1e-12 relative on the sum, which n <= 2^13 terms (these shapes)
keep: 2^13 2^-53 2 < 1e-12.

Inputs hold void labels of both sorts (-1 and >= C), a region whose score gap makes every other e_k exactly 0, and an exact
two-way tie; the host reference of every input is checked to fill both rows and three or more bins per metric."""
import ctypes

import numpy as np
import pytest
import torch

from modular_semantic_segmentation_amd.uncertainty_model import bin_index, confidence_tables_reference
from test_calibration_gpu import DEV, H, N, SENTINEL, W, _guard, _materialised, _scores, _tables, random_labels, random_scores
from test_calibration_gpu import ops  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

CLASSES = [2, 12, 13, 32]
TEMPS = [1.0, 0.5]
ALL = ('label', 'confidence', 'entropy', 'margin')
NLL_RTOL = 1e-12
M, O = 5, 24
BINS = O << M


def _host(tables):
    return {k: v.cpu().numpy() for k, v in tables.items()}


def _labels(like, c, seed):
    labels = random_labels(like, seed)
    labels[0, 0, :4] = (c, 255, -1, -5)                  # void of both sorts
    return labels


def _proves_something(want, c):
    """both rows and at least three bins per metric hold pixels"""
    for i in range(3):
        assert (want['hist'][i].sum(1) > 0).all(), i
        assert int((want['hist'][i].sum(0) > 0).sum()) >= 3, i


def _reference(maps, labels, c, **kwargs):
    return confidence_tables_reference(maps, maps['label'], labels, num_classes=c, mantissa_bits=M, octaves=O, **kwargs)


def _assert_tables(got, want, what):
    got = _host(got)
    assert np.array_equal(got['hist'], want['hist']), what
    assert np.array_equal(got['counts'], want['counts']), what
    return got


def _map_values(c, kind, shape=(N, H, W)):
    values = random_scores(c, 900 + c, *shape)
    a, b = (0, 1) if c == 2 else (1, c - 1)
    values[0, 0] = -200.0
    values[0, 0, :, a] = 0.0                              # a gap of 200: every other term is exactly 0
    values[0, 1, :, a] = values[0, 1, :, b] = 30.0       # an exact two-way tie at the top
    dev = torch.from_numpy(values).to(DEV)
    return torch.softmax(dev, -1).contiguous() if kind == 1 else dev


@pytest.mark.parametrize('kind', [0, 1], ids=['scores', 'probabilities'])
@pytest.mark.parametrize('c', CLASSES)
def test_materialised_map(ops, c, kind):
    source = _map_values(c, kind)
    labels_h = _labels(source.cpu().numpy(), c, 700 + c)
    labels = torch.from_numpy(labels_h).to(DEV)
    valid = (labels_h >= 0) & (labels_h < c)
    for T in TEMPS:
        maps = _host(ops.confidence_map(source, T, kind=kind, want=ALL))
        # (a probability map keeps ln(1e-20 + 0) finite, so only scores give terms of exactly 0)
        assert (maps['margin'] == 0).any() and (kind == 1 or ((maps['confidence'] == 1) & (maps['entropy'] == 0)).any())
        want = _reference(maps, labels_h, c)
        _proves_something(want, c)
        assert np.array_equal(want['counts'], np.bincount(labels_h[valid], minlength=c))
        tables = ops.confidence_stats(source, labels, T, kind=kind, mantissa_bits=M, octaves=O)
        got = _assert_tables(tables, want, (c, kind, T))
        # the tie (one row of W pixels, a tenth of them void): small_margin is exactly 1.0, in the bin of 1.0; the gap (another
        # row): entropy and least_confidence at most 2^-23, bin 0
        assert got['hist'][2][:, int(bin_index(np.float32([1.0]), M, O)[0])].sum() >= W // 2
        assert got['hist'][0][:, 0].sum() >= W // 2 and got['hist'][1][:, 0].sum() >= W // 2
        _, nll = ops.calibration_table(source, labels, [T], 10, kind=kind)
        ref = float(nll.cpu().numpy()[0])
        print('C=%d kind=%d T=%g: nll %.15g against the calibration table %.15g' % (c, kind, T, got['nll'].sum(), ref))
        assert abs(got['nll'].sum() - ref) <= NLL_RTOL * ref and (got['nll'][want['counts'] == 0] == 0).all()
        # two launches into the same tables add
        ops.confidence_stats(source, labels, T, kind=kind, mantissa_bits=M, octaves=O, tables=tables)
        twice = _host(tables)
        assert np.array_equal(twice['hist'], 2 * want['hist']) and np.array_equal(twice['counts'], 2 * want['counts'])
        assert abs(twice['nll'].sum() - 2 * ref) <= 2 * NLL_RTOL * ref
        # a fixed row: every pixel, no labels; with labels the NLL sums beside it
        for row in (0, 1):
            fixed = _host(ops.confidence_stats(source, None, T, kind=kind, fixed_row=row, mantissa_bits=M, octaves=O))
            want_row = _reference(maps, None, c, fixed_row=row)
            assert np.array_equal(fixed['hist'], want_row['hist']) and int(fixed['hist'][0][row].sum()) == labels_h.size
            assert not fixed['counts'].any() and not fixed['nll'].any() and not fixed['hist'][:, 1 - row].any()
        both = _host(ops.confidence_stats(source, labels, T, kind=kind, fixed_row=1, mantissa_bits=M, octaves=O))
        assert np.array_equal(both['hist'], want_row['hist']) and np.array_equal(both['counts'], want['counts'])


@pytest.mark.parametrize('m,o', [(3, 8), (8, 10), (4, 32)])
def test_other_bins(ops, m, o):
    c = 12
    source = _map_values(c, 0)
    labels_h = _labels(source.cpu().numpy(), c, 3)
    maps = _host(ops.confidence_map(source, 1.0, want=ALL))
    want = confidence_tables_reference(maps, maps['label'], labels_h, num_classes=c, mantissa_bits=m, octaves=o)
    got = ops.confidence_stats(source, torch.from_numpy(labels_h).to(DEV), 1.0, mantissa_bits=m, octaves=o)
    _assert_tables(got, want, (m, o))


def test_more_pixels_than_the_grid_takes_in_one_step(ops):
    """512 workgroups of 512 threads take 262 144 pixels a step: beyond it the grid-stride loop runs (two classes keep it small)"""
    c, shape = 2, (1, 1, 512 * 512 + 1000)
    source = torch.from_numpy(random_scores(c, 77, *shape)).to(DEV)
    labels_h = random_labels(source.cpu().numpy(), 78)
    maps = _host(ops.confidence_map(source, 1.0, want=ALL))
    want = _reference(maps, labels_h, c)
    _proves_something(want, c)
    _assert_tables(ops.confidence_stats(source, torch.from_numpy(labels_h).to(DEV), 1.0), want, 'stride')
    geo = (1, 64, 65)                                      # 266 240 output pixels
    S, bias = _scores(c, geo, 5, 2)
    maps = _host(ops.fused_head_multi_confidence(S, bias, *geo, c, 2, 1.0, want=ALL))
    labels_h = random_labels(np.zeros(maps['label'].shape + (c,), np.float32), 79)
    want = _reference(maps, labels_h, c)
    _proves_something(want, c)
    _assert_tables(ops.fused_head_multi_confidence_stats(S, bias, *geo, c, 2, torch.from_numpy(labels_h).to(DEV), 1.0), want, 'stride')


def _fused_inputs(c, geo, experts, mode):
    """scores with a region where class 0 leads by 300 (every other term exactly 0 in the experts' tables) and, in image 0, two
    classes tied in every expert; with more than two classes tables that treat those two alike, so that the fusion ties
    them too"""
    S, bias = _scores(c, geo, 40 + c + experts, experts)
    hi, wi = geo[1:]
    a, b = (0, 1) if c == 2 else (1, c - 1)
    for e, (s, bs) in enumerate(zip(S, bias)):
        s[0, 1:-1, 1:-1, a] += 8.0
        s[0, 1:-1, 1:-1, b] = s[0, 1:-1, 1:-1, a]
        s[-1, 1:-1, 1:3, 0] = 300.0
        # (beside it the experts disagree, so that a fusion of a few label tuples -- Bayes at two classes -- spreads too)
        noise = torch.Generator().manual_seed(7 * c + experts + 100 * e)
        s[-1, 1:-1, 3:-1, :c] += (4.0 * torch.randn((hi, wi - 2, c), generator=noise)).to(s.device)
        bs[b] = bs[a]
    tables = _tables(c, experts, mode, c + experts)
    for k, t in (tables if c > 2 else {}).items():       # (two classes alike would be all of them: the fusion would know nothing)
        t[..., b] = t[..., a]
        if k == 'tab':
            t[:, b, :] = t[:, a, :]
            t[:, b, b] = t[:, a, a]
            t[:, a, b] = t[:, a, a]
            t[:, b, a] = t[:, a, a]
        if k == 'logprior':
            t[a] = t[b] = t.max()
    return S, bias, tables


FUSED = [(e, m, c) for e in (2, 3, 4) for m in (0, 1, 2) for c in CLASSES]
GEOS = {'3x5': (N, H // 8, W // 8), '8x12': (3, 8, 12)}


def _check_fused(ops, experts, mode, c, geo, temps):
    n, hi, wi = geo
    S, bias, tables = _fused_inputs(c, geo, experts, mode)
    _, _, expert_scores = _materialised(ops, S, bias, geo, c, mode, tables)
    labels_h = _labels(np.zeros((n, 8 * hi, 8 * wi, c), np.float32), c, 50 + c)
    # (the winner's share of the labels: those of the first expert's map, so that both rows fill)
    first = expert_scores[0].argmax(-1).cpu().numpy()
    labels_h = np.where((labels_h >= 0) & (labels_h < c) & (np.arange(labels_h.size).reshape(labels_h.shape) % 2 == 0), first,
                        labels_h).astype(np.int32)
    labels = torch.from_numpy(labels_h).to(DEV)
    for T in temps:
        maps = _host(ops.fused_head_multi_confidence(S, bias, n, hi, wi, c, mode, T, want=ALL, **tables))
        # the tie reaches the mean always (equal probabilities); Bayes and Dirichlet where their tables let the two lead
        tied = bool((maps['margin'] == 0).any())
        print('E=%d mode=%d C=%d T=%g: the fused posterior holds an exact tie: %s' % (experts, mode, c, T, tied))
        assert tied or mode != 2
        want = _reference(maps, labels_h, c)
        _proves_something(want, c)
        got, got_experts = ops.fused_head_multi_confidence_stats(S, bias, n, hi, wi, c, mode, labels, T, mantissa_bits=M,
                                                                 octaves=O, experts=True, **tables)
        got = _assert_tables(got, want, (experts, mode, c, T))
        alone = ops.fused_head_multi_confidence_stats(S, bias, n, hi, wi, c, mode, labels, T, mantissa_bits=M, octaves=O, **tables)
        assert np.array_equal(_host(alone)['hist'], want['hist'])
        nll, enll = _calibration(ops, S, bias, geo, c, mode, labels, T, tables)
        assert abs(got['nll'].sum() - nll) <= NLL_RTOL * nll, (got['nll'].sum(), nll)
        got_experts = _host(got_experts)
        for e in range(experts):
            own = _host(ops.confidence_stats(expert_scores[e], labels, T, mantissa_bits=M, octaves=O))
            print('expert %d: %d counts differ between the head and the materialised kernel on its score map' % (
                e, int(np.abs(got_experts['hist'][e] - own['hist']).sum()) // 2))
            assert np.array_equal(got_experts['hist'][e], own['hist']) and np.array_equal(got_experts['counts'][e], own['counts'])
            assert abs(got_experts['nll'][e].sum() - enll[e]) <= NLL_RTOL * enll[e]
            assert abs(own['nll'].sum() - enll[e]) <= NLL_RTOL * enll[e]
            own_maps = _host(ops.confidence_map(expert_scores[e], T, want=('entropy', 'margin')))
            assert (own_maps['entropy'] == 0).any() and (own_maps['margin'] == 0).any()       # terms of exactly 0; an exact tie
        # fixed rows without labels, the experts' beside the fusion's; twice adds
        for row in (0, 1):
            t, et = ops.fused_head_multi_confidence_stats(S, bias, n, hi, wi, c, mode, None, T, fixed_row=row, mantissa_bits=M,
                                                          octaves=O, experts=True, **tables)
            ops.fused_head_multi_confidence_stats(S, bias, n, hi, wi, c, mode, None, T, fixed_row=row, mantissa_bits=M,
                                                  octaves=O, tables=t, expert_tables=et, **tables)
            want_row = _reference(maps, None, c, fixed_row=row)
            assert np.array_equal(_host(t)['hist'], 2 * want_row['hist']) and not _host(t)['counts'].any()
            et = _host(et)
            assert (et['hist'][:, :, row].sum(-1) == 2 * labels_h.size).all() and not et['hist'][:, :, 1 - row].any()


def _calibration(ops, S, bias, geo, c, mode, labels, T, tables):
    """(the fusion's NLL sum, every expert's) of the calibration head at one temperature"""
    n, hi, wi = geo
    _, nll, _, enll = ops.fused_head_multi_calibration(S, bias, n, hi, wi, c, mode, labels, [T], 10, experts=True, **tables)
    return float(nll.cpu().numpy()[0]), enll.cpu().numpy()[:, 0]


@pytest.mark.parametrize('experts,mode,c', FUSED, ids=['E%d-%s-C%d' % (e, 'bdm'[m], c) for e, m, c in FUSED])
def test_fused_launch(ops, experts, mode, c):
    _check_fused(ops, experts, mode, c, GEOS['3x5'], TEMPS)


@pytest.mark.parametrize('mode', [0, 1, 2], ids=['bayes', 'dirichlet', 'mean'])
def test_fused_launch_on_several_workgroups(ops, mode):
    _check_fused(ops, 3, mode, 12, GEOS['8x12'], TEMPS)


def test_refusals_leave_the_tables_untouched(ops):
    from modular_semantic_segmentation_amd import _lib
    from modular_semantic_segmentation_amd.ops import _ptr, _ptr_array
    c, geo = 12, GEOS['3x5']
    n, hi, wi = geo
    values = _map_values(c, 0)
    S, bias = _scores(c, geo, 3, 3)
    t = _tables(c, 3, 1, 3)
    labels = torch.zeros((N, H, W), dtype=torch.int32, device=DEV)
    bufs = {'hist': _guard((3, 2, BINS), torch.int64), 'nll': _guard((c,), torch.float64), 'counts': _guard((c,), torch.int64),
            'expert_hist': _guard((3, 3, 2, BINS), torch.int64), 'expert_nll': _guard((3, c), torch.float64),
            'expert_counts': _guard((3, c), torch.int64)}
    null = ctypes.c_void_p(0)

    def off(tensor, by):
        return ctypes.c_void_p(tensor.data_ptr() + by)
    how = dict(temperature=1.0, labels=_ptr(labels), mantissa_bits=M, octaves=O, fixed_row=-1, hist=_ptr(bufs['hist']),
               nll=_ptr(bufs['nll']), counts=_ptr(bufs['counts']))
    good = {'xv_confidence_stats': dict(dict(values=_ptr(values), kind=0, n=N, ppi=H * W, num_classes=c), **how),
            'xv_fused_head_multi_confidence_stats_fwd': dict(dict(
                S=_ptr_array(S), bias=_ptr_array(bias), num_experts=3, n=n, hi=hi, wi=wi, num_classes=c, mode=1, tab=_ptr(t['tab']),
                lognorm=_ptr(t['lognorm']), logprior=_ptr(t['logprior'])), **how, expert_hist=_ptr(bufs['expert_hist']),
                expert_nll=_ptr(bufs['expert_nll']), expert_counts=_ptr(bufs['expert_counts']))}
    shared = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('nan')), dict(temperature=float('inf')),
              dict(num_classes=1), dict(num_classes=33), dict(n=0), dict(mantissa_bits=2), dict(mantissa_bits=9), dict(octaves=7),
              dict(octaves=33), dict(fixed_row=-2), dict(fixed_row=2), dict(labels=null), dict(hist=null), dict(nll=null),
              dict(counts=null), dict(labels=off(labels, 2)), dict(hist=off(bufs['hist'], 4)), dict(nll=off(bufs['nll'], 4)),
              dict(counts=off(bufs['counts'], 4)),
              dict(mantissa_bits=8, octaves=11)]             # 6 x 2816 x 4 bytes and 16 C: one copy of one table above 64 KB
    only = {'xv_confidence_stats': [dict(kind=2), dict(kind=-1), dict(ppi=0), dict(values=null), dict(values=off(values, 2))],
            'xv_fused_head_multi_confidence_stats_fwd': [
                dict(mode=3), dict(mode=-1), dict(hi=0), dict(wi=-1), dict(num_experts=1), dict(num_experts=5), dict(S=None),
                dict(bias=None), dict(tab=null), dict(lognorm=null), dict(logprior=null), dict(mode=0, tab=null),
                dict(tab=off(t['tab'], 2)), dict(expert_hist=null), dict(expert_nll=null), dict(expert_counts=null),
                dict(expert_hist=null, expert_nll=null), dict(expert_hist=off(bufs['expert_hist'], 4)),
                dict(mantissa_bits=7, octaves=14)]}          # 43 KB a table: four of them and the fusion tables pass 160 KB
    for e in range(3):
        for name, tensors, by in (('S', S, None), ('S', S, 4), ('bias', bias, None), ('bias', bias, 2)):
            ptrs = [x.data_ptr() for x in tensors]
            ptrs[e] = 0 if by is None else ptrs[e] + by
            only['xv_fused_head_multi_confidence_stats_fwd'].append({name: (ctypes.c_void_p * 3)(*ptrs)})
    for entry, cases in only.items():
        for change in shared + cases:
            assert getattr(_lib.lib(), entry)(*dict(good[entry], **change).values(), null) == -1, (entry, change)
    torch.cuda.synchronize()
    assert all(bool((v == SENTINEL).all()) for v in bufs.values())
    # what fits: 64 KB exactly for one table without labels (mantissa 7, 21 octaves: 6 x 2688 x 4 = 63 KB) and the good calls
    assert _lib.lib().xv_confidence_stats(*dict(good['xv_confidence_stats'], mantissa_bits=7, octaves=21, fixed_row=0, labels=null,
                                                hist=_ptr(torch.zeros((3, 2, 2688), dtype=torch.int64, device=DEV))).values(),
                                          null) == 0
    for entry in good:
        assert getattr(_lib.lib(), entry)(*good[entry].values(), null) == 0, entry
    torch.cuda.synchronize()
    # the Python layer
    for kwargs in (dict(labels=labels[:1]), dict(tables={'hist': bufs['hist'][:2], 'nll': bufs['nll'], 'counts': bufs['counts']})):
        with pytest.raises(ValueError):
            ops.confidence_stats(values, **dict(dict(labels=labels), **kwargs))
    with pytest.raises(TypeError):
        ops.confidence_stats(values, labels.long())
    with pytest.raises(ValueError):
        ops.fused_head_multi_confidence_stats(S[:1], bias[:1], n, hi, wi, c, 2, labels)
    with pytest.raises(ValueError):
        ops.fused_head_multi_confidence_stats(S, bias, n, hi, wi, c, 1, labels, tab=t['tab'])
