"""Confidence maps without a GPU: calibration.confidence_reference on pixels worked by hand, calibration.risk_coverage on a
table whose curve is known by inspection, the two entry points of csrc/confidence.hip against the ABI conventions (as
tests/test_calibration_cpu.py restates them), what both refuse before anything calls into HIP, and the model methods with
`_build_experts` stubbed: the refusals with their reason, and fit_temperature storing the temperature a search names."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from modular_semantic_segmentation_amd import _lib
from modular_semantic_segmentation_amd.calibration import Q_ONE, confidence_reference, risk_coverage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_on_pixels_by_hand():
    l2, l3 = math.log(2.0), math.log(3.0)
    scores = np.array([[l2, 0.0, 0.0],          # probabilities (1/2, 1/4, 1/4)
                       [0.0, l3, l3],           # a tied maximum: (1/7, 3/7, 3/7), the first of the two wins
                       [5.0, 5.0, 5.0],         # all tied
                       [-200.0, 0.0, -200.0]])  # a spread of 200: the losers' terms vanish
    label, conf, entropy, margin = confidence_reference(scores, 1.0)
    assert label.tolist() == [0, 1, 0, 1] and label.dtype == np.int64
    assert conf == pytest.approx([0.5, 3 / 7, 1 / 3, 1.0], abs=1e-15)
    assert margin[:3] == pytest.approx([0.25, 0.0, 0.0], abs=1e-15) and margin[1] == 0.0 and margin[2] == 0.0
    assert margin[3] == pytest.approx(1.0, abs=1e-80)
    assert entropy[:3] == pytest.approx([1.5 * l2, math.log(7) - 6 / 7 * l3, l3], abs=1e-14)
    assert entropy[3] >= 0.0 and entropy[3] < 1e-80 and np.isfinite(entropy).all()
    # T = 1/2 squares the odds: (4/6, 1/6, 1/6); T = 2 takes their root
    _, c2, e2, m2 = confidence_reference(scores[:1], 0.5)
    assert c2[0] == pytest.approx(2 / 3, abs=1e-15) and m2[0] == pytest.approx(0.5, abs=1e-15)
    assert e2[0] == pytest.approx(-(2 / 3 * math.log(2 / 3) + 1 / 3 * math.log(1 / 6)), abs=1e-14)
    _, c3, _, _ = confidence_reference(scores[:1], 2.0)
    assert c3[0] == pytest.approx(math.sqrt(2) / (math.sqrt(2) + 2), abs=1e-15)
    # a spread beyond float64's exponent range: e_k = 0 exactly, and the term adds nothing
    far = confidence_reference(np.array([[0.0, -1e4]]), 1.0)
    assert far[1][0] == 1.0 and far[2][0] == 0.0 and far[3][0] == 1.0
    # probabilities (kind 1): the winner is the first maximum of the probabilities; a probability of exactly 0 stays finite
    p = np.array([[0.5, 0.25, 0.25], [0.0, 1.0, 0.0], [0.5, 0.5, 0.0]])
    label, conf, entropy, margin = confidence_reference(p, 1.0, kind=1)
    assert label.tolist() == [0, 1, 0]
    assert conf == pytest.approx([0.5, 1.0, 0.5], abs=1e-15) and margin == pytest.approx([0.25, 1.0, 0.0], abs=1e-15)
    assert np.isfinite(entropy).all() and entropy[2] == pytest.approx(l2, abs=1e-14)
    # leading axes are kept
    assert confidence_reference(np.zeros((2, 3, 4, 5)), 1.0)[1].shape == (2, 3, 4)
    for bad in (dict(temperature=0.0), dict(temperature=float('nan')), dict(temperature=float('inf')), dict(kind=2)):
        with pytest.raises(ValueError):
            confidence_reference(scores, **dict(dict(temperature=1.0), **bad))


def test_risk_coverage_by_inspection():
    """16 bins, 20 pixels: 10 in bin 15 (9 right), 6 in bin 8 (3 right), 4 in bin 5 (none right)"""
    t = np.zeros((16, 3), np.int64)
    t[15] = (10, 9, 10 * (Q_ONE * 15 // 16))
    t[8] = (6, 3, 6 * (Q_ONE // 2))
    t[5] = (4, 0, 4 * (Q_ONE * 5 // 16))
    rc = risk_coverage(t)
    assert rc['thresholds'].tolist() == [j / 16 for j in range(16)]
    assert rc['coverage'].tolist() == [1.0] * 6 + [0.8] * 3 + [0.5] * 7
    assert rc['risk'].tolist() == pytest.approx([0.4] * 6 + [0.25] * 3 + [0.1] * 7, abs=1e-15)
    # flat at 0.1 up to coverage 0.5, then the trapezoids to (0.8, 0.25) and (1, 0.4)
    assert rc['area'] == pytest.approx(0.05 + 0.3 * 0.175 + 0.2 * 0.325, abs=1e-15)
    # nothing in the upper bins: no risk there
    low = np.zeros((4, 3), np.int64)
    low[1] = (5, 5, 0)
    rc = risk_coverage(low)
    assert rc['coverage'].tolist() == [1.0, 1.0, 0.0, 0.0] and rc['risk'][:2].tolist() == [0.0, 0.0]
    assert np.isnan(rc['risk'][2:]).all() and rc['area'] == 0.0
    empty = risk_coverage(np.zeros((4, 3), np.int64))
    assert np.isnan(empty['coverage']).all() and np.isnan(empty['risk']).all() and math.isnan(empty['area'])
    for shape in ((16,), (16, 2), (2, 16, 3)):
        with pytest.raises(ValueError):
            risk_coverage(np.zeros(shape, np.int64))


def test_new_entry_points_follow_the_abi_conventions():
    from ctypes import POINTER, c_float, c_int, c_int64, c_void_p
    p, table = c_void_p, POINTER(c_void_p)
    assert _lib.SIGNATURES['xv_confidence_map'] == (
        c_int, [p, c_int, c_int, c_int64, c_int, c_float, c_float, c_int64, p, p, p, p, p])
    assert _lib.SIGNATURES['xv_fused_head_multi_confidence_fwd'] == (
        c_int, [table, table, c_int, c_int, c_int, c_int, c_int, c_int, p, p, p, c_float, c_float, c_int64, p, p, p, p, p])
    header = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(os.path.join(ROOT, 'include', 'xview_hip.h')).read(), flags=re.S)
    csrc = os.path.join(ROOT, 'modular_semantic_segmentation_amd', 'csrc')
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith('.hip')}
    assert '#include "xv_common.h"' in sources['confidence.hip'] and '#include "xv_conf.h"' in sources['confidence.hip']
    for name, nargs in (('xv_confidence_map', 13), ('xv_fused_head_multi_confidence_fwd', 19)):
        declared = re.findall(r'\bint\s+%s\s*\(([^()]*)\)\s*;' % name, header)
        assert len(declared) == 1 and len(declared[0].split(',')) == nargs == len(_lib.SIGNATURES[name][1]), name
        where = [(f, m) for f, text in sources.items()
                 for m in re.findall(r'extern "C"\s+int\s+%s\s*\(([^{;]*)\)\s*\{' % name, text)]
        assert [f for f, _ in where] == ['confidence.hip'], (name, where)
        assert len(where[0][1].split(',')) == nargs, name
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert 'confidence.hip' in re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()
    assert 'xv_conf.h' in re.search(r'^HDRS := (.*)$', mk, re.M).group(1).split()           # hashed into xv_source_hash()
    # the per-pixel arithmetic is written once, on the statements the calibration tables count by
    conf_h, calib_h = open(os.path.join(csrc, 'xv_conf.h')).read(), open(os.path.join(csrc, 'xv_calib.h')).read()
    assert len(re.findall(r'void conf_pixel\(', conf_h)) == 1 and sources['confidence.hip'].count('conf_pixel<CM>(') == 1
    assert sources['confidence.hip'].count('conf_store<CM>(') == 2                            # both kernels end in it
    for shared in ('calib_term(', 'calib_conf('):
        assert shared in conf_h and len(re.findall(r'float %s' % re.escape(shared), calib_h)) == 1
        assert shared in calib_h.split('void calib_pixel(')[1]                                # calib_pixel runs them too
    assert _lib.lib().xv_version() == 604                                                     # purely additive
    from modular_semantic_segmentation_amd import ops
    assert callable(ops.confidence_map) and callable(ops.fused_head_multi_confidence)


# ---- refused before anything calls into HIP: made-up aligned pointers that are never dereferenced (every case is refused) ---
EINVAL, ESHAPE = _lib.CONSTANTS['XV_EINVAL'], _lib.CONSTANTS['XV_ESHAPE']
BASE = 0x7f0000000000
PTR = {name: BASE + (i << 20) for i, name in enumerate(('values', 'tab', 'lognorm', 'logprior', 'label', 'conf', 'entropy',
                                                        'margin'))}
EXPERT = [BASE + ((32 + i) << 20) for i in range(5)]
BIAS = [BASE + ((48 + i) << 20) for i in range(5)]
OUTS = dict(temperature=1.0, threshold=0.0, void_label=-1, label_out=PTR['label'], conf_out=PTR['conf'],
            entropy_out=PTR['entropy'], margin_out=PTR['margin'], stream=None)
MAP_GOOD = dict(dict(values=PTR['values'], kind=0, n=1, ppi=960, num_classes=5), **OUTS)
FUSED_GOOD = dict(dict(S=EXPERT[:3], bias=BIAS[:3], num_experts=3, n=1, hi=3, wi=5, num_classes=5, mode=2, tab=None,
                       lognorm=None, logprior=None), **OUTS)
OUT_CASES = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('nan')), dict(temperature=float('inf')),
             dict(threshold=-0.25), dict(threshold=1.5), dict(threshold=float('nan')), dict(threshold=float('inf')),
             dict(num_classes=1), dict(num_classes=33), dict(n=0),
             dict(label_out=None, conf_out=None, entropy_out=None, margin_out=None),
             dict(label_out=PTR['label'] + 4), dict(conf_out=PTR['conf'] + 2), dict(entropy_out=PTR['entropy'] + 2),
             dict(margin_out=PTR['margin'] + 1)]
MAP_CASES = OUT_CASES + [dict(kind=2), dict(kind=-1), dict(ppi=0), dict(n=-1), dict(values=None), dict(values=PTR['values'] + 2)]
FUSED_CASES = OUT_CASES + [
    dict(mode=3), dict(mode=-1), dict(hi=0), dict(wi=0), dict(num_experts=1, S=EXPERT[:1], bias=BIAS[:1]),
    dict(num_experts=5, S=EXPERT[:5], bias=BIAS[:5]), dict(S=None), dict(bias=None),
    dict(S=[EXPERT[0], None, EXPERT[2]]), dict(S=[EXPERT[0], EXPERT[1] + 4, EXPERT[2]]),
    dict(bias=[BIAS[0], BIAS[1], BIAS[2] + 2]), dict(mode=0, tab=None, logprior=PTR['logprior']),
    dict(mode=0, tab=PTR['tab'], logprior=None), dict(mode=1, tab=PTR['tab'], lognorm=None, logprior=PTR['logprior']),
    dict(mode=1, tab=PTR['tab'] + 2, lognorm=PTR['lognorm'], logprior=PTR['logprior'])]


def _pointers(values):
    return None if values is None else (ctypes.c_void_p * len(values))(*values)


@pytest.mark.parametrize('change', MAP_CASES, ids=[','.join(c) + str(i) for i, c in enumerate(MAP_CASES)])
def test_the_map_entry_refuses_before_anything_calls_into_hip(change):
    assert _lib.lib().xv_confidence_map(*dict(MAP_GOOD, **change).values()) == EINVAL


@pytest.mark.parametrize('change', FUSED_CASES, ids=[','.join(c) + str(i) for i, c in enumerate(FUSED_CASES)])
def test_the_fused_entry_refuses_before_anything_calls_into_hip(change):
    args = dict(FUSED_GOOD, **change)
    call = [_pointers(v) if k in ('S', 'bias') else v for k, v in args.items()]
    assert _lib.lib().xv_fused_head_multi_confidence_fwd(*call) == EINVAL


def test_shapes_the_library_cannot_address_are_a_shape_error_after_every_argument_error():
    assert _lib.lib().xv_confidence_map(*dict(MAP_GOOD, ppi=1 << 41).values()) == ESHAPE
    assert _lib.lib().xv_confidence_map(*dict(MAP_GOOD, ppi=1 << 41, threshold=2.0).values()) == EINVAL
    for change, code in ((dict(hi=1 << 24), ESHAPE), (dict(hi=1 << 24, temperature=0.0), EINVAL), (dict(hi=1 << 24, mode=3), EINVAL)):
        call = [_pointers(v) if k in ('S', 'bias') else v for k, v in dict(FUSED_GOOD, **change).items()]
        assert _lib.lib().xv_fused_head_multi_confidence_fwd(*call) == code, change


# ---- the model methods ------------------------------------------------------------------------------------------------------
C = 12
DESC = ({'rgb': 'float32', 'depth': 'float32', 'labels': 'int32'},
        {'rgb': (None, None, 3), 'depth': (None, None, 1), 'labels': (None, None)}, C)
EXPERTS = dict(num_channels={'rgb': 3, 'depth': 1}, num_units=64, expert_model='fcn', device='cpu',
               modalities=['depth', 'rgb'])
CMS = {'depth': np.random.default_rng(0).integers(1, 50, (C, C)), 'rgb': np.random.default_rng(1).integers(1, 50, (C, C))}
DATA = {'rgb': np.zeros((1, 16, 16, 3), np.float32), 'depth': np.zeros((1, 16, 16, 1), np.float32),
        'labels': np.zeros((1, 16, 16), np.int32)}


def _no_experts(cls):
    class NoExperts(cls):
        def _build_experts(self):
            self.experts = {}
    return NoExperts


def test_models_that_have_no_class_scores_refuse_with_their_reason():
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
        with pytest.raises(NotImplementedError, match=word) as info:
            net.predict_confidence(DATA)
        assert net._calibration_refusal() in str(info.value) and 'predict_confidence' in str(info.value)
    served = _no_experts(BayesFusion)(data_description=DESC, confusion_matrices=CMS, **EXPERTS)
    for outputs in (('confidence', 'confidence'), ('label',), ('variance',)):
        with pytest.raises(ValueError):
            served.predict_confidence(DATA, outputs=outputs)


def test_fit_temperature_stores_the_best_temperature(monkeypatch):
    from modular_semantic_segmentation_amd.bayes_mix import BayesFusion
    net = _no_experts(BayesFusion)(data_description=DESC, confusion_matrices=CMS, **EXPERTS)
    asked = []

    def search(data, temperatures, **kwargs):
        asked.append(list(temperatures))
        return {'temperatures': list(temperatures), 'measures': [], 'tables': None, 'best': temperatures[3]}
    monkeypatch.setattr(net, 'calibration_search', search)
    assert 'temperature' not in net.config
    out = net.fit_temperature(DATA)
    assert asked[0] == pytest.approx(list(np.geomspace(0.25, 4.0, 9)), rel=1e-15) and len(asked[0]) == 9
    assert out['best'] == asked[0][3] and net.config['temperature'] == asked[0][3]
    net.fit_temperature(DATA, [0.5, 1.0, 2.0, 3.0])
    assert asked[1] == [0.5, 1.0, 2.0, 3.0] and net.config['temperature'] == 3.0
    # the stored temperature is the default of predict_confidence, an explicit one wins, and without either it is 1
    seen = []
    monkeypatch.setattr(net, '_confidence_batch', lambda batch, T, want, threshold, void_label: seen.append((T, want, threshold)) or {
        k: __import__('torch').zeros((1, 16, 16)) for k in want})
    out = net.predict_confidence(DATA, outputs=('margin',))
    assert sorted(out) == ['label', 'margin'] and out['label'].shape == (1, 16, 16)
    net.predict_confidence(DATA, temperature=0.75, threshold=0.5)
    del net.config['temperature']
    net.predict_confidence(DATA)
    assert seen == [(3.0, ('label', 'margin'), 0.0), (0.75, ('label', 'confidence'), 0.5), (1.0, ('label', 'confidence'), 0.0)]


def test_evaluate_confidence_prints_one_row_per_threshold(capsys):
    from modular_semantic_segmentation_amd import experiments
    from modular_semantic_segmentation_amd.calibration import calibration_measures
    t = np.zeros((16, 3), np.int64)
    t[15], t[8], t[5] = (10, 9, 10 * (Q_ONE * 15 // 16)), (6, 3, 6 * (Q_ONE // 2)), (4, 0, 4 * (Q_ONE * 5 // 16))

    class Net(object):
        config = {'temperature': 2.0}

        def score_calibration(self, data, temperature=1.0):
            assert temperature == 2.0
            return calibration_measures(t, 5.0), t
    out = experiments.evaluate_confidence(Net(), None, [0.0, 0.5, 0.55])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 4 and lines[0].startswith('temperature 2:')
    assert out['thresholds'].tolist() == [0.0, 0.5, 9 / 16] and out['coverage'].tolist() == [1.0, 0.8, 0.5]
    assert 'coverage 0.800 risk 0.2500' in lines[2] and 'coverage 0.500 risk 0.1000' in lines[3]
