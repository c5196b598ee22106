"""The fused head for three and four experts without a GPU: its declaration and ctypes signature, and which models the two
predicates (multi_head_applicable, fused_head_applicable) accept."""
import ctypes
import re

import pytest

from modular_semantic_segmentation_amd import _lib
from modular_semantic_segmentation_amd.basic_fusion_model import fused_head_applicable, multi_head_applicable
from modular_semantic_segmentation_amd.fcn import FcnEngine


def test_the_header_declares_the_entry_point():
    text = open(_lib.HEADER).read()
    m = re.search(r'int\s+xv_fused_head_multi_fwd\s*\(([^)]*)\)\s*;', text)
    assert m, 'include/xview_hip.h does not declare xv_fused_head_multi_fwd'
    names = [p.split()[-1].lstrip('*') for p in m.group(1).split(',')]
    assert names == ['S', 'bias', 'num_experts', 'n', 'hi', 'wi', 'num_classes', 'mode', 'tab', 'lognorm', 'logprior',
                     'fused_label', 'stream']


def test_the_ctypes_signature_follows_the_declaration():
    res, args = _lib.SIGNATURES['xv_fused_head_multi_fwd']
    assert res is ctypes.c_int and len(args) == 13
    table = ctypes.POINTER(ctypes.c_void_p)                       # a host array of device pointers
    assert args[:2] == [table, table]
    assert args[2:8] == [ctypes.c_int] * 6
    assert args[8:] == [ctypes.c_void_p] * 5


def test_ops_names_the_entry_point():
    from modular_semantic_segmentation_amd import ops
    assert callable(ops.fused_head_multi)
    assert ops.FUSED_HEAD_MODES == {'bayes': 0, 'dirichlet': 1, 'mean': 2}


def _fcn(commuted=True):
    eng = FcnEngine.__new__(FcnEngine)                            # (no device: the predicates only ask the head's form)
    eng.affine = {} if commuted else {'upscore': None}
    eng.dense_deconv = {}
    return eng


class _Stub(object):
    def __init__(self, experts, **config):
        self.modalities = list(experts)
        self.experts = experts
        self.config = config


def _stub(n, **config):
    return _Stub({'m%d' % i: _fcn() for i in range(n)}, **config)


@pytest.mark.parametrize('n,expected', [(2, False), (3, True), (4, True), (5, False)])
def test_multi_head_applicable_by_the_number_of_experts(n, expected):
    assert multi_head_applicable(_stub(n)) is expected


def test_multi_head_applicable_refusals():
    assert multi_head_applicable(_stub(3, fused_head=True))
    assert not multi_head_applicable(_stub(3, fused_head=False))
    other = _Stub({'a': _fcn(), 'b': object(), 'c': _fcn()})      # an expert that is no FcnEngine
    assert not multi_head_applicable(other)
    affine = _Stub({'a': _fcn(), 'b': _fcn(commuted=False), 'c': _fcn()})     # a head that does not commute
    assert not multi_head_applicable(affine)


def test_fused_head_applicable_stays_two_expert():
    assert fused_head_applicable(_stub(2))
    assert not fused_head_applicable(_stub(3))
    assert not fused_head_applicable(_stub(4))
