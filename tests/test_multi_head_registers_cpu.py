"""Register budget of the fused head for two to four experts (tools/occupancy_scan.py, as
tests/test_fused_average_registers_cpu.py pins its sibling): every instantiation exists once and has no scratch, and at 12
classes each mode holds at least the waves per SIMD the same scan reports for its two-expert sibling -- the budget is the
siblings', not a fixed number."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

CLASS_STEPS = [4, 8, 12, 16, 20, 24, 28, 32]


@pytest.fixture(scope='module')
def scan():
    import occupancy_scan
    return occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'heads.hip'))


@pytest.fixture(scope='module')
def rows(scan):
    return [r for r in scan if 'fused_head_multi_kernel' in r[0]]


def test_every_instantiation_exists_once(rows):
    """<CM, MODE, FULL>: eight class steps, three modes, the run-time and the full class count"""
    keys = sorted(tuple(int(v) for v in re.search(r'ILi(\d+)ELi(\d)ELb(\d)E', r[0]).groups()) for r in rows)
    assert keys == sorted((cm, mode, full) for cm in CLASS_STEPS for mode in (0, 1, 2) for full in (0, 1))


def test_no_scratch_anywhere(rows):
    for kern, regs, scratch, waves in rows:
        assert scratch == 0 and waves >= 1, '%s: %d registers, %d B scratch' % (kern, regs, scratch)


def _one(scan, pattern):
    found = [r for r in scan if re.search(pattern, r[0])]
    assert len(found) == 1, (pattern, found)
    return found[0]


@pytest.mark.parametrize('full', [0, 1], ids=['runtime', 'full'])
@pytest.mark.parametrize('mode', [0, 1, 2], ids=['bayes', 'dirichlet', 'mean'])
def test_twelve_classes_hold_the_siblings_waves(scan, mode, full):
    mine = _one(scan, r'fused_head_multi_kernelILi12ELi%dELb%dE' % (mode, full))
    if mode == 2:
        sibling = _one(scan, r'fused_head_average_kernelILi12ELb0ELb%dE' % full)
    else:
        sibling = _one(scan, r'fused_head_kernelILi12ELi%dELb%dE' % (mode, full))
    assert mine[2] == 0 and sibling[2] == 0
    assert mine[3] >= sibling[3], '%s: %d waves per SIMD (%d registers) against %d (%d registers) of %s' % (
        mine[0], mine[3], mine[1], sibling[3], sibling[1], sibling[0])
