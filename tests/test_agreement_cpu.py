"""The expert-agreement table without a GPU: agreement_measures on hand-written tables whose every measure is known by
inspection, and the two entry points of csrc/agreement.hip against the ABI conventions (declared in the header, derived into
_lib.SIGNATURES, defined once with the declared parameter counts), as tests/test_grouped_score_cpu.py restates them for its own."""
import math
import os
import re

import numpy as np
import pytest

from modular_semantic_segmentation_amd import _lib
from modular_semantic_segmentation_amd.basic_fusion_model import agreement_measures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _two_expert_table():
    """3 classes, class 0 without pixels; 20 pixels in all.  mask bit 0 = expert 'a' right, bit 1 = expert 'b' right."""
    t = np.zeros((3, 4, 2, 3), np.int64)
    t[1, 3, 1, 0] = 8        # both right, unanimous, fused right
    t[1, 1, 0, 0] = 3        # a alone right, fused right: follows a
    t[1, 1, 0, 1] = 1        # a alone right, fused wrong with some expert: that is b
    t[1, 2, 0, 0] = 2        # b alone right, fused right: follows b
    t[2, 0, 1, 1] = 2        # both wrong and unanimous, fused with them
    t[2, 0, 1, 0] = 1        # both wrong and unanimous, fused right: rescued
    t[2, 0, 0, 1] = 1        # both wrong, different labels, fused with one of them: the table does not say which
    t[2, 0, 0, 2] = 1        # both wrong, different labels, fused with neither: its own way
    t[2, 3, 1, 2] = 1        # both right, fused wrong on its own: lost
    return t


def test_two_experts_every_measure_by_inspection():
    m = agreement_measures(_two_expert_table(), ['a', 'b'])
    assert m['pixels'] == 20
    assert m['fused_accuracy'] == (8 + 3 + 2 + 1) / 20
    assert m['expert_accuracy'] == {'a': (8 + 3 + 1 + 1) / 20, 'b': (8 + 2 + 1) / 20}
    assert m['best_expert_accuracy'] == 13 / 20
    assert m['oracle_accuracy'] == (8 + 3 + 1 + 2 + 1) / 20
    assert m['unanimous'] == (8 + 2 + 1 + 1) / 20
    assert m['fused_accuracy_on_disagreement'] == (3 + 2) / 8
    assert m['rescued'] == 1 / 20
    assert m['lost'] == (1 + 1) / 20
    assert m['own_way_errors'] == (1 + 1) / 20
    assert m['follows'] == {'a': 3 / 8, 'b': (2 + 1) / 8} and m['follows_undecided'] == 1 / 8
    per = m['per_class']
    assert per['pixels'].tolist() == [0, 14, 6]
    assert math.isnan(per['fused_accuracy'][0]) and per['fused_accuracy'][1:].tolist() == [13 / 14, 1 / 6]
    assert math.isnan(per['expert_accuracy']['a'][0]) and per['expert_accuracy']['a'][1:].tolist() == [12 / 14, 1 / 6]
    assert per['expert_accuracy']['b'][1:].tolist() == [10 / 14, 1 / 6]
    assert per['rescued'][1:].tolist() == [0, 1 / 6] and per['lost'][1:].tolist() == [1 / 14, 1 / 6]
    assert per['unanimous'][1:].tolist() == [8 / 14, 4 / 6] and math.isnan(per['unanimous'][0])
    assert per['fused_accuracy_on_disagreement'][1:].tolist() == [5 / 6, 0.0]
    assert per['follows']['a'][1:].tolist() == [3 / 6, 0.0] and per['follows']['b'][1:].tolist() == [3 / 6, 0.0]
    assert per['follows_undecided'][1:].tolist() == [0.0, 1 / 2]
    assert per['best_expert_accuracy'][1:].tolist() == [12 / 14, 1 / 6] and math.isnan(per['best_expert_accuracy'][0])
    assert per['own_way_errors'][1:].tolist() == [0.0, 2 / 6] and per['oracle_accuracy'][1:].tolist() == [1.0, 1 / 6]


def test_three_experts_have_no_follows():
    t = np.zeros((2, 8, 2, 3), np.int64)
    t[0, 7, 1, 0] = 5        # all right
    t[0, 5, 0, 0] = 2        # experts 0 and 2 right, fused right
    t[1, 2, 0, 1] = 2        # expert 1 alone right, fused with a wrong one
    t[1, 0, 0, 2] = 1        # nobody right, fused on its own
    m = agreement_measures(t)
    assert 'follows' not in m and 'follows_undecided' not in m and 'follows' not in m['per_class']
    assert m['pixels'] == 10 and m['fused_accuracy'] == 0.7
    assert m['expert_accuracy'] == {0: 0.7, 1: 0.7, 2: 0.7} and m['best_expert_accuracy'] == 0.7
    assert m['oracle_accuracy'] == 0.9 and m['unanimous'] == 0.5 and m['fused_accuracy_on_disagreement'] == 2 / 5
    assert m['rescued'] == 0.0 and m['lost'] == 0.2 and m['own_way_errors'] == 0.1
    named = agreement_measures(t, ['rgb', 'depth', 'ir'])
    assert list(named['expert_accuracy']) == ['rgb', 'depth', 'ir']
    assert named['per_class']['expert_accuracy']['depth'].tolist() == [5 / 7, 2 / 3]


def test_no_disagreement_and_no_pixels_give_nan():
    t = np.zeros((2, 4, 2, 3), np.int64)
    t[1, 3, 1, 0] = 4
    m = agreement_measures(t, ['a', 'b'])
    assert m['unanimous'] == 1.0 and math.isnan(m['fused_accuracy_on_disagreement']) and math.isnan(m['follows']['a'])
    empty = agreement_measures(np.zeros((2, 16, 2, 3), np.int64))
    assert empty['pixels'] == 0 and math.isnan(empty['fused_accuracy']) and len(empty['expert_accuracy']) == 4


def test_measures_refuse_other_shapes():
    for shape in ((3, 4, 2), (3, 5, 2, 3), (3, 32, 2, 3), (3, 4, 3, 2)):
        with pytest.raises(ValueError):
            agreement_measures(np.zeros(shape, np.int64))
    with pytest.raises(ValueError):
        agreement_measures(np.zeros((3, 4, 2, 3), np.int64), ['a', 'b', 'c'])


def test_evaluate_agreement_prints_the_overall_measures(capsys):
    from modular_semantic_segmentation_amd import experiments

    class Net(object):
        def score_agreement(self, data):
            return agreement_measures(_two_expert_table(), ['a', 'b']), _two_expert_table()
    measures, table = experiments.evaluate_agreement(Net(), None)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == 'fused accuracy 0.700 best expert 0.650 oracle 0.750'
    assert lines[1].split() == ['a:', '0.650', 'accuracy'] and len(lines) == 7 and 'rescued 0.0500 lost 0.1000' in lines[4]
    assert np.array_equal(table, _two_expert_table()) and measures['pixels'] == 20
    experiments.evaluate_agreement(Net(), None, print_results=False)
    assert capsys.readouterr().out == ''


def test_new_entry_points_follow_the_abi_conventions():
    from ctypes import POINTER, c_int, c_int64, c_void_p
    p, table = c_void_p, POINTER(c_void_p)
    assert _lib.SIGNATURES['xv_fused_head_multi_agreement_fwd'] == (
        c_int, [table, table, c_int, c_int, c_int, c_int, c_int, c_int, p, p, p, p, p, c_int, p, c_int, p])
    assert _lib.SIGNATURES['xv_agreement_table'] == (c_int, [p, table, c_int, p, p, c_int, c_int64, c_int, c_int, p, p])
    header = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(os.path.join(ROOT, 'include', 'xview_hip.h')).read(), flags=re.S)
    csrc = os.path.join(ROOT, 'modular_semantic_segmentation_amd', 'csrc')
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith('.hip')}
    assert '#include "xv_common.h"' in sources['agreement.hip']
    for name, nargs in (('xv_fused_head_multi_agreement_fwd', 17), ('xv_agreement_table', 11)):
        declared = re.findall(r'\bint\s+%s\s*\(([^()]*)\)\s*;' % name, header)
        assert len(declared) == 1 and len(declared[0].split(',')) == nargs == len(_lib.SIGNATURES[name][1]), name
        where = [(f, m) for f, text in sources.items()
                 for m in re.findall(r'extern "C"\s+int\s+%s\s*\(([^{;]*)\)\s*\{' % name, text)]
        assert [f for f, _ in where] == ['agreement.hip'], (name, where)
        assert len(where[0][1].split(',')) == nargs, name
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert 'agreement.hip' in re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()
    assert len(re.findall(r'xv_version\(void\)\s*\{\s*return 604;', ''.join(sources.values()))) == 1
    from modular_semantic_segmentation_amd import ops
    assert callable(ops.fused_head_multi_agreement) and callable(ops.agreement_table)
