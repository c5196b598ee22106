"""The uncertainty benchmarks of a posterior without a GPU: uncertainty_model.confidence_tables_reference -- the definition of
what csrc/confidence_stats.hip counts -- on pixels made by hand, the public methods of UncertaintyBenchmarks on a stub model
that provides the state hooks, the two entry points against the header and the ctypes table, what both refuse before anything
calls into HIP, and the models that refuse with their calibration refusal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from modular_semantic_segmentation_amd import _lib, ops
from modular_semantic_segmentation_amd import uncertainty_model as um
from modular_semantic_segmentation_amd.calibration import confidence_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, O = 5, 24
BINS = O << M
ONE_BIN = 23 * 32                                         # the bin of 1.0: (127 - (128 - 24)) << 5


def _maps(scores, temperature=1.0):
    label, conf, entropy, margin = confidence_reference(np.asarray(scores, np.float64), temperature)
    return {'label': label, 'confidence': conf.astype(np.float32), 'entropy': entropy.astype(np.float32),
            'margin': margin.astype(np.float32)}


def test_reference_on_pixels_by_hand():
    assert ops.CONFIDENCE_METRICS == um.CONFIDENCE_METRICS == ('entropy', 'least_confidence', 'small_margin')
    assert int(um.bin_index(np.float32([1.0]), M, O)[0]) == ONE_BIN
    scores = np.array([[0.0, -1e4, -1e4],                 # one-hot: conf 1, entropy 0, margin 1
                       [2.0, 2.0, -1e4],                  # an exact two-way tie: margin 0
                       [1.0, 0.0, 0.0],
                       [0.0, 0.5, 3.0],
                       [0.0, 0.5, 3.0],
                       [0.0, 0.5, 3.0]])
    maps = _maps(scores)
    assert maps['label'].tolist() == [0, 0, 0, 2, 2, 2] and maps['margin'][1] == 0 and maps['entropy'][0] == 0
    labels = np.array([0, 1, 0, 2, -1, 3], np.int32)      # right, wrong, right, right, void, void (>= C)
    t = um.confidence_tables_reference(maps, maps['label'], labels, num_classes=3)
    assert t['hist'].shape == (3, 2, BINS) and t['hist'].dtype == np.int64
    assert t['hist'].sum((1, 2)).tolist() == [4, 4, 4] and t['hist'][:, 1].sum(1).tolist() == [1, 1, 1]
    assert t['counts'].tolist() == [2, 1, 1] and not t['nll'].any()
    # the one-hot pixel: entropy 0 and least_confidence 0, both in bin 0 of the right row; its small_margin 0 too
    assert t['hist'][0][0][0] == 1 and t['hist'][1][0][0] == 1 and t['hist'][2][0][0] == 1
    # the tie, misclassified: small_margin is exactly 1.0, alone in the bin of 1.0
    assert np.float32(1.0) - maps['margin'][1] == 1.0
    assert t['hist'][2][1][ONE_BIN] == 1 and t['hist'][2][:, ONE_BIN].sum() == 1 and t['hist'][2][:, ONE_BIN + 1:].sum() == 0
    assert t['hist'][1][1][int(um.bin_index(np.float32([0.5]), M, O)[0])] == 1     # its least_confidence is 1 - 1/2
    # a fixed row counts the void pixels too and needs no labels
    for row in (0, 1):
        f = um.confidence_tables_reference(maps, maps['label'], None, num_classes=3, fixed_row=row)
        assert f['hist'][:, row].sum(1).tolist() == [6, 6, 6] and not f['hist'][:, 1 - row].any() and not f['counts'].any()
    g = um.confidence_tables_reference(maps, maps['label'], labels, num_classes=3, fixed_row=1)
    assert g['hist'][:, 1].sum(1).tolist() == [6, 6, 6] and g['counts'].tolist() == [2, 1, 1]
    # the NLL terms go to the ground-truth class of the valid pixels; two calls add
    nll = np.arange(1, 7, dtype=np.float32)
    a = um.confidence_tables_reference(maps, maps['label'], labels, nll_pixel=nll, num_classes=3)
    assert a['nll'].tolist() == [1.0 + 3.0, 2.0, 4.0]
    b = um.confidence_tables_reference(maps, maps['label'], labels, nll_pixel=nll, tables=a)
    assert b is a and np.array_equal(a['hist'], 2 * t['hist']) and a['counts'].tolist() == [4, 2, 2] and a['nll'].tolist() == [8.0, 4.0, 8.0]
    # values at or below 2^(1 - octaves) share bin 0; other bins
    tiny = {'entropy': np.float32([2.0 ** -23, 2.0 ** -30, 2.0 ** -22]), 'confidence': np.float32([1, 1, 1]),
            'margin': np.float32([1, 1, 1])}
    low = um.confidence_tables_reference(tiny, [0, 0, 0], None, num_classes=2, fixed_row=0)['hist'][0][0]
    assert low[0] == 2 and low[1 << M] == 1 and low.sum() == 3
    assert um.confidence_tables_reference(maps, maps['label'], labels, num_classes=3, mantissa_bits=3, octaves=8)['hist'].shape == (3, 2, 64)
    for bad in (dict(fixed_row=2), dict(labels=None), dict(mantissa_bits=9), dict(num_classes=None)):
        kwargs = dict(dict(labels=labels, num_classes=3), **bad)
        with pytest.raises(ValueError):
            um.confidence_tables_reference(maps, maps['label'], kwargs.pop('labels'), **kwargs)


class Stub(um.UncertaintyBenchmarks):
    """a model whose batches already carry their maps: the state hooks on the host, the tables on the CPU"""
    uncertainty_metrics = um.CONFIDENCE_METRICS
    device = torch.device('cpu')

    def __init__(self, **config):
        self.config = dict({'num_classes': 3, 'batchsize': 2}, **config)
        self.states = 0

    def _device_batches(self, batches, labels):
        return batches

    def _to_device(self, array, dtype):
        return torch.from_numpy(np.ascontiguousarray(array)).to(dtype)

    def _uncertainty_state(self, batch):
        self.states += 1
        return batch

    def _uncertainty_accumulate(self, state, labels, tables, temperature, fixed_row):
        maps = {'entropy': state['entropy'] * np.float32(temperature), 'confidence': state['confidence'], 'margin': state['margin']}
        t = um.confidence_tables_reference(maps, state['win'], None if labels is None else labels.numpy(),
                                           nll_pixel=state['entropy'], num_classes=3, fixed_row=fixed_row)
        for k in t:
            tables[k] += torch.from_numpy(t[k])


def _data(separable):
    rng = np.random.default_rng(0)
    n = 8
    labels = rng.integers(0, 3, (n, 4, 4)).astype(np.int32)
    win = labels.copy()
    win[:, :2] = (labels[:, :2] + 1) % 3                   # the upper half of every image is wrong
    labels[:, 0, 0] = -1
    unc = rng.random((n, 4, 4)).astype(np.float32) * 0.25
    if separable:
        unc[:, :2] += 0.5                                 # every wrong pixel above every right one
    else:
        unc[:, :2] = unc[:, 2:]                           # the wrong pixels carry the values of the right ones
        labels[:, 0, 0], labels[:, 2, 0] = -1, -1
    return {'entropy': unc, 'confidence': 1 - unc, 'margin': 1 - unc, 'win': win, 'labels': labels}


def test_public_methods_through_the_hooks():
    net = Stub()
    for metric in um.CONFIDENCE_METRICS:
        assert net.misclassification_detection_score(_data(True), metric)[2] == 1.0
        assert net.misclassification_detection_score(_data(False), metric)[2] == 0.5
        assert net.out_of_distribution_detection_score(_data(True), metric, _data(True))[2] == 0.5
        counts, edges = net.value_distribution(_data(True), metric)
        assert counts.sum() == 8 * 15 and len(edges) == BINS + 1
    t = net.uncertainty_tables(_data(True))
    assert t['metrics'] == um.CONFIDENCE_METRICS and t['hist'].shape == (3, 2, BINS) and int(t['counts'].sum()) == 8 * 15
    nll, counts = net.nll_score(_data(True))
    assert np.array_equal(counts, t['counts']) and np.allclose(nll, t['nll_sum'] / t['counts'])
    # labels are not read by the out-of-distribution benchmark
    bare = {k: v for k, v in _data(True).items() if k != 'labels'}
    shifted = dict(bare, entropy=bare['entropy'] + 1)
    assert net.out_of_distribution_detection_score(bare, 'entropy', shifted)[2] == 1.0
    assert net.uncertainty_tables(bare, fixed_row=1)['hist'][0][1].sum() == 8 * 16
    with pytest.raises(ValueError, match='labels'):
        net.uncertainty_tables(bare)
    # a search obtains every batch's state once and accumulates it per temperature
    net.states = 0
    search = net.temperature_search(_data(True), [1.0, 2.0, 4.0])
    assert net.states == 4 and [s['temperature'] for s in search] == [1.0, 2.0, 4.0]
    for s in search:
        net.config['temperature_scaling'] = s['temperature']
        assert np.array_equal(s['tables']['hist'], net.uncertainty_tables(_data(True))['hist'])
    with pytest.raises(UserWarning):
        net.misclassification_detection_score(_data(True), 'variance')
    with pytest.raises(ValueError, match='experts'):
        net.uncertainty_tables(_data(True), experts=True)


def test_class_relations_and_default_temperature():
    from modular_semantic_segmentation_amd.base_model import BaseModel
    from modular_semantic_segmentation_amd.basic_fusion_model import FusionModel
    from modular_semantic_segmentation_amd.bayesian_fcn import BayesianFCN
    assert issubclass(BaseModel, um.UncertaintyBenchmarks) and issubclass(um.UncertaintyModel, um.UncertaintyBenchmarks)
    assert BaseModel.uncertainty_metrics == FusionModel.uncertainty_metrics == ops.CONFIDENCE_METRICS
    assert BayesianFCN.uncertainty_metrics == ops.UNCERTAINTY_METRICS
    for name in ('_uncertainty_state', '_uncertainty_accumulate', '_default_temperature', '_uncertainty_check', '_uncertainty_experts'):
        assert getattr(BayesianFCN, name) is not getattr(BaseModel, name), name           # the mixin's answers come first
    for name in ('misclassification_detection_score', 'out_of_distribution_detection_score', 'nll_score', 'value_distribution',
                 'uncertainty_tables', 'temperature_search'):
        assert getattr(FusionModel, name) is getattr(um.UncertaintyBenchmarks, name) is getattr(BayesianFCN, name), name
    net = BaseModel.__new__(BaseModel)
    net.config = {}
    assert net._temperature() == 1.0 and net._temperature(3) == 3.0
    net.config['temperature'] = 2.0
    assert net._temperature() == 2.0
    net.config['temperature_scaling'] = 0.5
    assert net._temperature() == 0.5
    bayesian = BayesianFCN.__new__(BayesianFCN)
    bayesian.config = {'temperature': 2.0}
    assert bayesian._temperature() == 1.0                                                   # as before: temperature_scaling alone


# ---- the entry points -------------------------------------------------------------------------------------------------------
def test_new_entry_points_follow_the_abi_conventions():
    from ctypes import POINTER, c_float, c_int, c_int64, c_void_p
    p, table = c_void_p, POINTER(c_void_p)
    assert _lib.SIGNATURES['xv_confidence_stats'] == (
        c_int, [p, c_int, c_int, c_int64, c_int, c_float, p, c_int, c_int, c_int, p, p, p, p])
    assert _lib.SIGNATURES['xv_fused_head_multi_confidence_stats_fwd'] == (
        c_int, [table, table, c_int, c_int, c_int, c_int, c_int, c_int, p, p, p, c_float, p, c_int, c_int, c_int, p, p, p, p, p,
                p, p])
    header = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(os.path.join(ROOT, 'include', 'xview_hip.h')).read(), flags=re.S)
    csrc = os.path.join(ROOT, 'modular_semantic_segmentation_amd', 'csrc')
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith('.hip')}
    for name, nargs in (('xv_confidence_stats', 14), ('xv_fused_head_multi_confidence_stats_fwd', 23)):
        declared = re.findall(r'\bint\s+%s\s*\(([^()]*)\)\s*;' % name, header)
        assert len(declared) == 1 and len(declared[0].split(',')) == nargs == len(_lib.SIGNATURES[name][1]), name
        where = [(f, m) for f, text in sources.items()
                 for m in re.findall(r'extern "C"\s+int\s+%s\s*\(([^{;]*)\)\s*\{' % name, text)]
        assert [f for f, _ in where] == ['confidence_stats.hip'], (name, where)
        assert callable(getattr(_lib.lib(), name))
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert 'confidence_stats.hip' in re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()
    assert 'xv_conf_stats.h' in re.search(r'^HDRS := (.*)$', mk, re.M).group(1).split()     # hashed into xv_source_hash()
    # the count of a pixel is written once, on conf_pixel and calib_pixel; both kernels call it and nothing else
    stats_h, src = open(os.path.join(csrc, 'xv_conf_stats.h')).read(), sources['confidence_stats.hip']
    assert len(re.findall(r'void conf_stats_pixel\(', stats_h)) == 1 and stats_h.count('conf_pixel<CM>(') == 1
    assert src.count('conf_stats_pixel<CM>(') == 3 and 'conf_pixel<CM>(' not in src.replace('conf_stats_pixel<CM>(', '')
    assert 'xv_fast_exp' not in src and 'xv_fast_exp' not in stats_h                          # no arithmetic of its own
    assert _lib.lib().xv_version() == 604                                                     # purely additive
    assert callable(ops.confidence_stats) and callable(ops.fused_head_multi_confidence_stats)


EINVAL, ESHAPE = _lib.CONSTANTS['XV_EINVAL'], _lib.CONSTANTS['XV_ESHAPE']
BASE = 0x7f0000000000
PTR = {name: BASE + (i << 24) for i, name in enumerate(('values', 'tab', 'lognorm', 'logprior', 'labels', 'hist', 'nll', 'counts',
                                                        'expert_hist', 'expert_nll', 'expert_counts'))}
EXPERT = [BASE + ((32 + i) << 24) for i in range(5)]
BIAS = [BASE + ((48 + i) << 24) for i in range(5)]
HOW = dict(temperature=1.0, labels=PTR['labels'], mantissa_bits=5, octaves=24, fixed_row=-1, hist=PTR['hist'], nll=PTR['nll'],
           counts=PTR['counts'])
MAP_GOOD = dict(dict(values=PTR['values'], kind=0, n=1, ppi=960, num_classes=5), **HOW, stream=None)
FUSED_GOOD = dict(dict(S=EXPERT[:3], bias=BIAS[:3], num_experts=3, n=1, hi=3, wi=5, num_classes=5, mode=2, tab=None,
                       lognorm=None, logprior=None), **HOW, expert_hist=PTR['expert_hist'], expert_nll=PTR['expert_nll'],
                  expert_counts=PTR['expert_counts'], stream=None)
HOW_CASES = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('nan')), dict(temperature=float('inf')),
             dict(num_classes=1), dict(num_classes=33), dict(n=0), dict(mantissa_bits=2), dict(mantissa_bits=9), dict(octaves=7),
             dict(octaves=33), dict(fixed_row=-2), dict(fixed_row=2), dict(labels=None), dict(hist=None), dict(nll=None),
             dict(counts=None), dict(fixed_row=0, nll=None), dict(labels=PTR['labels'] + 2), dict(hist=PTR['hist'] + 4),
             dict(nll=PTR['nll'] + 4), dict(counts=PTR['counts'] + 4), dict(mantissa_bits=8, octaves=11),
             dict(mantissa_bits=8, octaves=32)]
MAP_CASES = HOW_CASES + [dict(kind=2), dict(kind=-1), dict(ppi=0), dict(n=-1), dict(values=None), dict(values=PTR['values'] + 2)]
FUSED_CASES = HOW_CASES + [
    dict(mode=3), dict(mode=-1), dict(hi=0), dict(wi=0), dict(num_experts=1, S=EXPERT[:1], bias=BIAS[:1]),
    dict(num_experts=5, S=EXPERT[:5], bias=BIAS[:5]), dict(S=None), dict(bias=None),
    dict(S=[EXPERT[0], None, EXPERT[2]]), dict(S=[EXPERT[0], EXPERT[1] + 4, EXPERT[2]]),
    dict(bias=[BIAS[0], BIAS[1], BIAS[2] + 2]), dict(mode=0, tab=None, logprior=PTR['logprior']),
    dict(mode=1, tab=PTR['tab'], lognorm=None, logprior=PTR['logprior']),
    dict(expert_hist=None), dict(expert_nll=None), dict(expert_counts=None), dict(expert_hist=None, expert_counts=None),
    dict(expert_nll=PTR['expert_nll'] + 4), dict(mantissa_bits=7, octaves=14)]      # four tables of 43 KB pass 160 KB


def _pointers(values):
    return None if values is None else (ctypes.c_void_p * len(values))(*values)


@pytest.mark.parametrize('change', MAP_CASES, ids=[','.join(c) + str(i) for i, c in enumerate(MAP_CASES)])
def test_the_map_entry_refuses_before_anything_calls_into_hip(change):
    assert _lib.lib().xv_confidence_stats(*dict(MAP_GOOD, **change).values()) == EINVAL


@pytest.mark.parametrize('change', FUSED_CASES, ids=[','.join(c) + str(i) for i, c in enumerate(FUSED_CASES)])
def test_the_fused_entry_refuses_before_anything_calls_into_hip(change):
    args = dict(FUSED_GOOD, **change)
    call = [_pointers(v) if k in ('S', 'bias') else v for k, v in args.items()]
    assert _lib.lib().xv_fused_head_multi_confidence_stats_fwd(*call) == EINVAL


def test_shapes_the_library_cannot_address_are_a_shape_error_after_every_argument_error():
    assert _lib.lib().xv_confidence_stats(*dict(MAP_GOOD, ppi=1 << 41).values()) == ESHAPE
    assert _lib.lib().xv_confidence_stats(*dict(MAP_GOOD, ppi=1 << 41, octaves=40).values()) == EINVAL
    for change, code in ((dict(hi=1 << 24), ESHAPE), (dict(hi=1 << 24, temperature=0.0), EINVAL), (dict(hi=1 << 24, mode=3), EINVAL)):
        call = [_pointers(v) if k in ('S', 'bias') else v for k, v in dict(FUSED_GOOD, **change).items()]
        assert _lib.lib().xv_fused_head_multi_confidence_stats_fwd(*call) == code, change


# ---- the model methods ------------------------------------------------------------------------------------------------------
def test_models_that_have_no_class_scores_refuse_with_their_reason():
    from test_confidence_cpu import CMS, DATA, DESC, EXPERTS, _no_experts
    from modular_semantic_segmentation_amd.bayes_mix import BayesFusion
    from modular_semantic_segmentation_amd.ibcc_mix import IbccFusion
    from modular_semantic_segmentation_amd.variance_mix import VarianceFusion
    from modular_semantic_segmentation_amd.uncertainty_dirichlet_mix import UncertaintyMix
    nets = [(_no_experts(BayesFusion)(data_description=DESC, confusion_matrices=CMS, decision_matrix=True, **EXPERTS), 'lookup'),
            (_no_experts(IbccFusion)(data_description=DESC, confusion_matrices=CMS, **EXPERTS), 'lookup'),
            (_no_experts(VarianceFusion)(data_description=DESC, dropout_rate=0.5, num_samples=5, **EXPERTS), 'dropout'),
            (_no_experts(UncertaintyMix)(data_description=DESC, class_prior='uniform', delta=1e-2, beta=1e-2, dropout_rate=0.5,
                                         num_samples=5, **EXPERTS), 'dropout')]
    for net, word in nets:
        for call in (lambda: net.uncertainty_tables(DATA), lambda: net.misclassification_detection_score(DATA, 'entropy'),
                     lambda: net.out_of_distribution_detection_score(DATA, 'small_margin', DATA), lambda: net.nll_score(DATA),
                     lambda: net.value_distribution(DATA, 'least_confidence'), lambda: net.temperature_search(DATA, [1.0, 2.0])):
            with pytest.raises(NotImplementedError, match=word) as info:
                call()
            assert net._calibration_refusal() in str(info.value)
    served = _no_experts(BayesFusion)(data_description=DESC, confusion_matrices=CMS, **EXPERTS)
    assert served._calibration_refusal() is None and served._uncertainty_experts() == served.modalities
    with pytest.raises(UserWarning):
        served.misclassification_detection_score(DATA, 'variance')
