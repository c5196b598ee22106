"""Calibration scoring without a GPU: calibration_measures on hand-built tables whose every measure is known by inspection,
regroup, table_reference on ten pixels written out by hand, the capacity against the LDS arithmetic, the three entry points of
csrc/calibration.hip against the ABI conventions (as tests/test_agreement_cpu.py restates them), and the model-level refusals
with `_build_experts` stubbed."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from modular_semantic_segmentation_amd import _lib
from modular_semantic_segmentation_amd.calibration import (Q_ONE, best_temperature, calibration_measures, regroup,
                                                           table_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand_table():
    """16 fine bins, 20 pixels, every confidence a dyadic number: 10 pixels at 15/16 (9 right), 6 at 1/2 (3 right), 4 at 5/16
    (none right)"""
    t = np.zeros((16, 3), np.int64)
    t[15] = (10, 9, 10 * (Q_ONE * 15 // 16))
    t[8] = (6, 3, 6 * (Q_ONE // 2))
    t[5] = (4, 0, 4 * (Q_ONE * 5 // 16))
    return t


def test_measures_by_inspection():
    for bins in (16, 4):                                   # (4 coarse bins keep the three groups apart)
        m = calibration_measures(_hand_table(), 5.0, num_bins=bins)
        assert m['pixels'] == 20 and m['accuracy'] == 12 / 20
        assert m['mean_confidence'] == pytest.approx((10 * 15 / 16 + 3 + 4 * 5 / 16) / 20, abs=1e-15)
        assert m['overconfidence'] == pytest.approx(13.625 / 20 - 0.6, abs=1e-15)
        assert m['ECE'] == pytest.approx((10 * (15 / 16 - 0.9) + 0 + 4 * 5 / 16) / 20, abs=1e-15)
        assert m['MCE'] == pytest.approx(5 / 16, abs=1e-15) and m['NLL'] == 0.25
        d = m['diagram']
        assert d['edges'].tolist() == [j / bins for j in range(bins + 1)] and int(d['count'].sum()) == 20
        top = bins - 1
        assert d['count'][top] == 10 and d['accuracy'][top] == 0.9 and d['confidence'][top] == 15 / 16
        assert math.isnan(d['accuracy'][0]) and math.isnan(d['confidence'][0])
    # two coarse bins: [0, 1/2) holds the 4 pixels, [1/2, 1] the other 16 (12 right, confidence 12.375 / 16)
    m = calibration_measures(_hand_table(), 5.0, num_bins=2)
    assert m['ECE'] == pytest.approx((4 * 5 / 16 + 16 * (12.375 / 16 - 0.75)) / 20, abs=1e-15)
    assert m['MCE'] == pytest.approx(5 / 16, abs=1e-15) and m['diagram']['count'].tolist() == [4, 16]


def test_measures_of_an_empty_table_and_other_shapes():
    m = calibration_measures(np.zeros((16, 3), np.int64), 0.0)
    assert m['pixels'] == 0 and math.isnan(m['ECE']) and math.isnan(m['accuracy']) and math.isnan(m['NLL'])
    for shape in ((16,), (16, 2), (2, 16, 3)):
        with pytest.raises(ValueError):
            calibration_measures(np.zeros(shape, np.int64), 0.0)
    assert best_temperature([0.5, 1.0, 2.0], [{'NLL': 0.4}, {'NLL': 0.3}, {'NLL': 0.3}]) == 1.0


def test_regroup():
    t = np.random.default_rng(0).integers(0, 1 << 40, (2, 1024, 3))
    assert np.array_equal(regroup(t, 16), t.reshape(2, 16, 64, 3).sum(2))            # exact: 16 divides 1024
    assert np.array_equal(regroup(t, 1024), t)
    r15 = regroup(t[0], 15)
    want = np.zeros((15, 3), np.int64)
    for b in range(1024):
        want[b * 15 // 1024] += t[0, b]
    assert np.array_equal(r15, want) and np.array_equal(r15.sum(0), t[0].sum(0))
    for bins in (0, 1025):
        with pytest.raises(ValueError):
            regroup(t, bins)


def test_reference_on_ten_pixels_by_hand():
    """Two classes: a pixel with scores (ln a, 0) has confidence a / (a + 1) at T = 1 and a^2 / (a^2 + 1) at T = 1/2."""
    l2, l9 = math.log(2.0), math.log(9.0)
    scores = np.array([[[l2, 0], [l2, 0], [0, l9], [0, 0], [l9, 0]],
                       [[0, l2], [0, l2], [l9, 0], [0, 0], [l2, 0]]])
    labels = np.array([[0, 1, 1, 0, -1], [1, 2, 1, 1, 255]])          # -1, 2 (= C) and 255 count nothing
    table, nll, conf = table_reference(scores, labels, [1.0, 0.5], 4)
    assert table.shape == (2, 16, 3) and nll.shape == (2,) and conf.shape == (2, 2, 5)

    def q(fr):
        return int(fr * Q_ONE)                                        # (exact: a Fraction)
    c23, c910, c45, c8182 = Fraction(2, 3), Fraction(9, 10), Fraction(4, 5), Fraction(81, 82)
    want = np.zeros((2, 16, 3), np.int64)
    # T = 1: three pixels at 2/3 (bin 10; two right), two at 9/10 (bin 14; one right), two at 1/2 (bin 8; one right)
    want[0, 10] = (3, 2, 3 * q(c23))
    want[0, 14] = (2, 1, 2 * q(c910))
    want[0, 8] = (2, 1, 2 * (Q_ONE // 2))
    # T = 1/2: 4/5 (bin 12), 81/82 (bin 15), 1/2 stays
    want[1, 12] = (3, 2, 3 * q(c45))
    want[1, 15] = (2, 1, 2 * q(c8182))
    want[1, 8] = (2, 1, 2 * (Q_ONE // 2))
    assert np.array_equal(table, want)
    assert nll[0] == pytest.approx(-(2 * math.log(2 / 3) + math.log(1 / 3) + math.log(0.9) + math.log(0.1) + 2 * math.log(0.5)),
                                   abs=1e-12)
    assert nll[1] == pytest.approx(-(2 * math.log(0.8) + math.log(0.2) + math.log(81 / 82) + math.log(1 / 82)
                                     + 2 * math.log(0.5)), abs=1e-12)
    assert conf[0, 0].tolist() == pytest.approx([2 / 3, 2 / 3, 0.9, 0.5, 0.9], abs=1e-15)
    assert conf[1, 1].tolist() == pytest.approx([0.8, 0.8, 81 / 82, 0.5, 0.8], abs=1e-15)
    # groups: image 0 in group 1, image 1 out of range
    gt, gn, _ = table_reference(scores, labels, [1.0], 4, groups=[1, 5], num_groups=2)
    one, one_nll, _ = table_reference(scores[:1], labels[:1], [1.0], 4)
    assert gt.shape == (2, 1, 16, 3) and not gt[0].any() and np.array_equal(gt[1], one) and gn[0, 0] == 0 and gn[1, 0] == one_nll[0]
    # probabilities (kind 1): the same pixels as softmax rows give the same integers
    p = np.exp(scores) / np.exp(scores).sum(-1, keepdims=True)
    pt, pn, _ = table_reference(p, labels, [1.0, 0.5], 4, kind=1)
    assert np.array_equal(pt[..., :2], want[..., :2]) and np.abs(pt[..., 2] - want[..., 2]).max() <= 2
    assert pn == pytest.approx(nll, abs=1e-9)
    # the clip: a wrong pixel at confidence 1 costs -ln 1e-10, not 200
    _, big, _ = table_reference(np.array([[[0.0, -200.0]]]), np.array([[1]]), [1.0], 4)
    assert big[0] == pytest.approx(-math.log(1e-10), abs=1e-12)
    for bad in (dict(bin_bits=3), dict(bin_bits=11), dict(temperatures=[0.0]), dict(temperatures=[float('nan')]), dict(kind=2)):
        with pytest.raises(ValueError):
            table_reference(scores, labels, **dict(dict(temperatures=[1.0], bin_bits=4), **bad))


def test_capacity_is_the_lds_arithmetic():
    cap = _lib.lib().xv_calibration_capacity
    for bits in range(4, 11):
        for tables in range(1, 6):
            per = tables * (16 * (1 << bits) + 32 * 8)               # 16-byte cells, 32 double copies of the NLL sum
            assert cap(bits, tables) == min(16, (160 - 20) * 1024 // per), (bits, tables)
            assert cap(bits, tables) >= 1
    assert cap(10, 1) == 8 and cap(10, 3) == 2 and cap(10, 5) == 1 and cap(4, 1) == 16
    for bits, tables in ((3, 1), (11, 1), (10, 0), (10, 6), (-1, 1)):
        assert cap(bits, tables) == 0


def test_new_entry_points_follow_the_abi_conventions():
    from ctypes import POINTER, c_int, c_int64, c_void_p
    p, table = c_void_p, POINTER(c_void_p)
    assert _lib.SIGNATURES['xv_calibration_capacity'] == (c_int, [c_int, c_int])
    assert _lib.SIGNATURES['xv_calibration_table'] == (
        c_int, [p, c_int, p, p, c_int, c_int64, c_int, p, c_int, c_int, c_int, p, p, p])
    assert _lib.SIGNATURES['xv_fused_head_multi_calibration_fwd'] == (
        c_int, [table, table, c_int, c_int, c_int, c_int, c_int, c_int, p, p, p, p, p, c_int, p, c_int, c_int, p, p, p, p,
                c_int, p])
    header = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(os.path.join(ROOT, 'include', 'xview_hip.h')).read(), flags=re.S)
    csrc = os.path.join(ROOT, 'modular_semantic_segmentation_amd', 'csrc')
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith('.hip')}
    assert '#include "xv_common.h"' in sources['calibration.hip'] and '#include "xv_calib.h"' in sources['calibration.hip']
    for name, nargs in (('xv_calibration_capacity', 2), ('xv_calibration_table', 14),
                        ('xv_fused_head_multi_calibration_fwd', 23)):
        declared = re.findall(r'\bint\s+%s\s*\(([^()]*)\)\s*;' % name, header)
        assert len(declared) == 1 and len(declared[0].split(',')) == nargs == len(_lib.SIGNATURES[name][1]), name
        where = [(f, m) for f, text in sources.items()
                 for m in re.findall(r'extern "C"\s+int\s+%s\s*\(([^{;]*)\)\s*\{' % name, text)]
        assert [f for f, _ in where] == ['calibration.hip'], (name, where)
        assert len(where[0][1].split(',')) == nargs, name
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert 'calibration.hip' in re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()
    assert 'xv_calib.h' in re.search(r'^HDRS := (.*)$', mk, re.M).group(1).split()          # hashed into xv_source_hash()
    # the per-pixel arithmetic is written once, in the header both kernels call
    assert len(re.findall(r'void calib_pixel\(', open(os.path.join(csrc, 'xv_calib.h')).read())) == 1
    assert sources['calibration.hip'].count('calib_pixel<CM>(') == 1 and sources['calibration.hip'].count('calib_count<CM>(') == 3
    from modular_semantic_segmentation_amd import ops
    assert callable(ops.calibration_capacity) and callable(ops.calibration_table) and callable(ops.fused_head_multi_calibration)


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


def test_models_that_have_no_class_scores_refuse_with_a_reason():
    from modular_semantic_segmentation_amd.bayes_mix import BayesFusion
    from modular_semantic_segmentation_amd.ibcc_mix import IbccFusion
    from modular_semantic_segmentation_amd.variance_mix import VarianceFusion
    from modular_semantic_segmentation_amd.uncertainty_dirichlet_mix import UncertaintyMix
    from modular_semantic_segmentation_amd.bayesian_fcn import BayesianFCN
    nets = [(_no_experts(BayesFusion)(data_description=DESC, confusion_matrices=CMS, decision_matrix=True, **EXPERTS), 'lookup'),
            (_no_experts(IbccFusion)(data_description=DESC, confusion_matrices=CMS, **EXPERTS), 'lookup'),
            (_no_experts(VarianceFusion)(data_description=DESC, dropout_rate=0.5, num_samples=5, **EXPERTS), 'dropout'),
            (_no_experts(UncertaintyMix)(data_description=DESC, class_prior='uniform', delta=1e-2, beta=1e-2, dropout_rate=0.5,
                                         num_samples=5, **EXPERTS), 'dropout')]
    for net, word in nets:
        for call in (lambda: net.score_calibration(DATA), lambda: net.score_calibration(DATA, groups='image'),
                     lambda: net.calibration_search(DATA, [0.5, 1.0])):
            with pytest.raises(NotImplementedError, match=word):
                call()
    assert 'dropout' in BayesianFCN.calibration_refusal
    # the per-pixel Bayes fusion is served: no refusal before a device is needed
    assert _no_experts(BayesFusion)(data_description=DESC, confusion_matrices=CMS, **EXPERTS)._calibration_refusal() is None


def test_evaluate_calibration_prints_one_row_per_expert_and_the_fusion(capsys):
    from modular_semantic_segmentation_amd import experiments
    measures = calibration_measures(_hand_table(), 5.0)

    class Net(object):
        modalities = ['rgb', 'depth']

        def score_calibration(self, data, experts=False):
            assert experts
            return measures, _hand_table(), {m: (measures, _hand_table()) for m in self.modalities}

        def calibration_search(self, data, temperatures):
            return {'temperatures': [0.5, 2.0], 'measures': [measures, dict(measures, NLL=0.125)], 'best': 2.0}
    out = experiments.evaluate_calibration(Net(), None, temperatures=[0.5, 2.0])
    lines = capsys.readouterr().out.splitlines()
    assert [ln.split(':')[0].strip() for ln in lines] == ['rgb', 'depth', 'fusion', 'best temperature 2']
    assert 'accuracy 0.600 confidence 0.681 ECE 0.081' in lines[2] and 'NLL 0.2500' in lines[2] and 'NLL 0.1250' in lines[3]
    assert len(out) == 4 and out[3]['best'] == 2.0
    experiments.evaluate_calibration(Net(), None, print_results=False)
    assert capsys.readouterr().out == ''
