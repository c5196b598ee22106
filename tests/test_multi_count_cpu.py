"""The counting head for two to four experts without a GPU: its two declarations in the C header and the ctypes signatures
_lib derives from them, the op, and FusionComparison's route gate on stubs (as tests/test_multi_head_cpu.py builds them)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'xview_hip.h')


def _declaration(name):
    text = open(HEADER).read()
    m = re.search(r'^int %s\(([^;]*)\);' % name, text, re.M)
    assert m, name
    return [' '.join(p.split()) for p in m.group(1).replace('\n', ' ').split(',')]


def test_count_declaration_and_parameter_names():
    params = _declaration('xv_fused_head_multi_count_fwd')
    assert params == ['const float* const* S', 'const float* const* bias', 'int num_experts', 'int n', 'int hi', 'int wi',
                      'int num_classes', 'int mode', 'int num_points', 'const float* tab', 'const float* lognorm',
                      'const float* logprior', 'const int32_t* labels', 'const int32_t* group', 'int num_groups', 'int64_t* cm',
                      'int64_t* expert_cm', 'int max_workgroups', 'void* stream']


def test_capacity_declaration_and_parameter_names():
    assert _declaration('xv_fused_head_multi_count_capacity') == ['int num_classes', 'int num_experts', 'int mode']


def test_ctypes_signatures_follow_the_header():
    from modular_semantic_segmentation_amd import _lib
    res, args = _lib.SIGNATURES['xv_fused_head_multi_count_fwd']
    table = ctypes.POINTER(ctypes.c_void_p)                       # a host array of device pointers
    assert res is ctypes.c_int and len(args) == 19
    assert args[:2] == [table, table] and args[2:9] == [ctypes.c_int] * 7
    assert args[9:14] == [ctypes.c_void_p] * 5 and args[14] is ctypes.c_int
    assert args[15:17] == [ctypes.c_void_p] * 2 and args[17] is ctypes.c_int and args[18] is ctypes.c_void_p
    res, args = _lib.SIGNATURES['xv_fused_head_multi_count_capacity']
    assert res is ctypes.c_int and args == [ctypes.c_int] * 3


def test_ops_exist():
    from modular_semantic_segmentation_amd import ops
    assert callable(ops.fused_head_multi_count) and callable(ops.fused_head_multi_count_capacity)


def _fcn(commuted=True):
    from modular_semantic_segmentation_amd.fcn import FcnEngine
    eng = FcnEngine.__new__(FcnEngine)                            # (no device: the predicates only ask the head's form)
    eng.affine = {} if commuted else {'upscore': None}
    eng.dense_deconv = {}
    return eng


def _stub(experts, num_classes=12, fused_head=True, commuted=True, fcn=True):
    from modular_semantic_segmentation_amd.fusion_comparison import FusionComparison
    model = FusionComparison.__new__(FusionComparison)
    model.modalities = ['m%d' % i for i in range(experts)]
    model.config = {'num_classes': num_classes, 'fused_head': fused_head}
    model.experts = {m: (_fcn(commuted) if fcn else object()) for m in model.modalities}
    return model


@pytest.mark.parametrize('experts, expected', [(2, True), (3, True), (4, True), (5, False)])
def test_one_pass_heads_by_expert_count(experts, expected):
    assert _stub(experts).one_pass_heads_applicable() is expected


def test_one_pass_heads_refusals():
    assert _stub(3, fused_head=False).one_pass_heads_applicable() is False
    assert _stub(3, commuted=False).one_pass_heads_applicable() is False
    assert _stub(4, fcn=False).one_pass_heads_applicable() is False
    assert _stub(2, num_classes=21).one_pass_heads_applicable() is False       # the joint histogram's class limit
    assert _stub(3, num_classes=21).one_pass_heads_applicable() is True        # no such limit on the counting head
