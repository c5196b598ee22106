"""What the multi-expert entry points of the C ABI refuse, and with which code, without a GPU: every argument check of these
entry points returns before anything calls into HIP.  The device pointers are made-up aligned integers that are never
dereferenced, because EVERY case here is a refused one (an accepted call would launch on them)."""
import ctypes

import pytest

from modular_semantic_segmentation_amd import _lib

EINVAL, ESHAPE = _lib.CONSTANTS['XV_EINVAL'], _lib.CONSTANTS['XV_ESHAPE']

BASE = 0x7f0000000000            # 16-byte aligned, 1 MiB apart: nothing is ever read through them
PTR = {name: BASE + (i << 20) for i, name in enumerate(
    ('tab', 'lognorm', 'logprior', 'labels', 'group', 'out', 'out2', 'out3', 'out4', 'lut', 'fused', 'values'))}
EXPERT = [BASE + ((32 + i) << 20) for i in range(5)]      # S[e] (or the experts' label maps)
BIAS = [BASE + ((48 + i) << 20) for i in range(5)]
TEMPS = (ctypes.c_float * 16)(*([1.0] * 16))              # host memory: the one array the checks do read

# the arguments of a call that would pass (three experts, 5 classes, the mean: no tables, no groups); never made as it stands
GOOD = dict(S=EXPERT[:3], bias=BIAS[:3], num_experts=3, n=1, hi=3, wi=5, ppi=64 * 15, num_classes=5, mode=2, kind=0, num_points=1,
            tab=None, lognorm=None, logprior=None, labels=PTR['labels'], group=None, num_groups=1, lut=PTR['lut'],
            fused=PTR['fused'], values=PTR['values'], out=PTR['out'], out2=PTR['out2'], expert_out=None, expert_out2=None,
            temperatures=ctypes.cast(TEMPS, ctypes.c_void_p), num_temperatures=1, bin_bits=6, max_workgroups=0, stream=None)

HEAD = ['S', 'bias', 'num_experts', 'n', 'hi', 'wi', 'num_classes']
TABLES = ['tab', 'lognorm', 'logprior']
ENTRIES = {
    'xv_fused_head_multi_fwd': HEAD + ['mode'] + TABLES + ['out', 'stream'],
    'xv_fused_head_multi_count_fwd': HEAD + ['mode', 'num_points'] + TABLES + ['labels', 'group', 'num_groups', 'out', 'expert_out',
                                                                             'max_workgroups', 'stream'],
    'xv_fused_head_multi_agreement_fwd': HEAD + ['mode'] + TABLES + ['labels', 'group', 'num_groups', 'out', 'max_workgroups',
                                                                    'stream'],
    'xv_fused_head_multi_calibration_fwd': HEAD + ['mode'] + TABLES + ['labels', 'group', 'num_groups', 'temperatures',
                                                                      'num_temperatures', 'bin_bits', 'out', 'out2', 'expert_out',
                                                                      'expert_out2', 'max_workgroups', 'stream'],
    'xv_fused_head_multi_tuple_hist_fwd': HEAD + ['group', 'num_groups', 'out', 'max_workgroups', 'stream'],
    'xv_fused_head_multi_lut_count_fwd': HEAD + ['lut', 'labels', 'group', 'num_groups', 'out', 'max_workgroups', 'stream'],
    'xv_fused_head_multi_lut_fwd': HEAD + ['lut', 'out', 'stream'],
    # (S stands for the experts' label maps here: the same rules with 8-byte alignment)
    'xv_agreement_table': ['labels', 'S', 'num_experts', 'fused', 'group', 'n', 'ppi', 'num_classes', 'num_groups', 'out', 'stream'],
    'xv_calibration_table': ['values', 'kind', 'labels', 'group', 'n', 'ppi', 'num_classes', 'temperatures', 'num_temperatures',
                             'bin_bits', 'num_groups', 'out', 'out2', 'stream'],
}
TUPLE = ('xv_fused_head_multi_tuple_hist_fwd', 'xv_fused_head_multi_lut_count_fwd', 'xv_fused_head_multi_lut_fwd')


def _edit(values, index, delta):
    """values with entry `index` moved by `delta` bytes (None: made null)"""
    out = list(values)
    out[index] = None if delta is None else out[index] + delta
    return out


# (name, the arguments it changes, the code); a case applies to an entry that has every argument it names -- but for `bias`,
# which the cases that change the expert count carry along for the entries that have one
CASES = [
    ('one_expert', dict(num_experts=1, S=EXPERT[:1], bias=BIAS[:1]), EINVAL),
    ('five_experts', dict(num_experts=5, S=EXPERT[:5], bias=BIAS[:5]), EINVAL),
    ('one_class', dict(num_classes=1), EINVAL),
    ('33_classes', dict(num_classes=33), EINVAL),
    ('no_images', dict(n=0), EINVAL),
    ('null_S', dict(S=None), EINVAL),
    ('null_S1', dict(S=_edit(EXPERT[:3], 1, None)), EINVAL),
    ('S1_four_bytes_off', dict(S=_edit(EXPERT[:3], 1, 4)), EINVAL),
    ('bias2_two_bytes_off', dict(bias=_edit(BIAS[:3], 2, 2)), EINVAL),
    ('mode_3', dict(mode=3), EINVAL),
    ('bayes_without_tab', dict(mode=0, tab=None, logprior=PTR['logprior']), EINVAL),
    ('dirichlet_without_lognorm', dict(mode=1, tab=PTR['tab'], lognorm=None, logprior=PTR['logprior']), EINVAL),
    ('no_groups', dict(num_groups=0), EINVAL),
    ('two_groups_null_group', dict(num_groups=2, group=None), EINVAL),
    ('negative_max_workgroups', dict(max_workgroups=-1), EINVAL),
    ('hi_2_24', dict(hi=1 << 24), ESHAPE),
    ('ppi_2_41', dict(ppi=1 << 41), ESHAPE),
    # an argument rule and a shape rule broken together: the argument wins
    ('hi_2_24_and_bias2_two_bytes_off', dict(hi=1 << 24, bias=_edit(BIAS[:3], 2, 2)), EINVAL),
    ('hi_2_24_and_mode_3', dict(hi=1 << 24, mode=3), EINVAL),
    ('hi_2_24_and_no_groups', dict(hi=1 << 24, num_groups=0), EINVAL),
    ('ppi_2_41_and_no_groups', dict(ppi=1 << 41, num_groups=0), EINVAL),
]
# 32 classes with four experts: 2^20 tuples, more than the label-tuple heads hold -- a shape; with a null S[1] an argument
TUPLE_CASES = [
    ('32_classes_four_experts', dict(num_classes=32, num_experts=4, S=EXPERT[:4], bias=BIAS[:4]), ESHAPE),
    ('32_classes_four_experts_and_null_S1', dict(num_classes=32, num_experts=4, S=_edit(EXPERT[:4], 1, None), bias=BIAS[:4]), EINVAL),
]

PARAMS = [pytest.param(entry, change, code, id='%s-%s' % (entry, name))
          for entry, names in ENTRIES.items()
          for name, change, code in CASES + (TUPLE_CASES if entry in TUPLE else [])
          if all(k in names for k in change if k != 'bias' or 'num_experts' not in change)]


def _pointer_array(values):
    return None if values is None else (ctypes.c_void_p * len(values))(*values)


@pytest.mark.parametrize('entry,change,code', PARAMS)
def test_refused_before_anything_calls_into_hip(entry, change, code):
    args = dict(GOOD, **{k: v for k, v in change.items() if k in ENTRIES[entry]})
    call = [_pointer_array(args[k]) if k in ('S', 'bias') else args[k] for k in ENTRIES[entry]]
    assert getattr(_lib.lib(), entry)(*call) == code


def test_every_listed_case_is_exercised():
    """the table above reaches every entry point with every case the entry has the arguments for"""
    seen = {p.id for p in PARAMS}
    assert len(seen) == len(PARAMS)
    for entry, names in ENTRIES.items():
        assert '%s-no_images' % entry in seen
        assert ('%s-no_groups' % entry in seen) == ('num_groups' in names)
        assert ('%s-null_S1' % entry in seen) == ('S' in names)
        for case in ('one_expert', 'five_experts'):
            assert ('%s-%s' % (entry, case) in seen) == ('num_experts' in names)
        assert ('%s-mode_3' % entry in seen) == ('mode' in names)
        assert ('%s-32_classes_four_experts' % entry in seen) == (entry in TUPLE)
