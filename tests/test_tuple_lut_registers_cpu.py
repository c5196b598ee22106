"""Register budget of the label-tuple heads (csrc/tuple_lut.hip) from tools/occupancy_scan.py, as
tests/test_agreement_registers_cpu.py holds the agreement kernels': every instantiation of the three kernels exists once, none
has scratch, and each holds at least two waves per SIMD -- what a 512-thread workgroup of the counting kernels is (their tuple
histogram can take a whole CU's LDS: one workgroup per CU, those two waves are all the residency there is), and the floor of
the 256-thread lookup head too."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

CLASS_STEPS = [4, 8, 12, 16, 20, 24, 28, 32]
# waves per SIMD at 12 classes as the scan reports them: the histogram (73 registers), the counting lookup (75), the lookup
# head at four pixels per thread (126, held to four waves as fused_head_multi_kernel's Bayes mode)
PINNED_12 = {'hist': 6, 'count': 6, 'lut': 4}
# the least any instantiation may hold: a 512-thread workgroup IS two waves per SIMD; the 256-thread lookup head is held to the
# same two (its 20- to 32-class forms use 174 to 247 registers: two waves, and one step more would halve its residency)
WORKGROUP_WAVES = 2


@pytest.fixture(scope='module')
def scan():
    import occupancy_scan
    return occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'tuple_lut.hip'))


def _key(row):
    """(kernel form, padded class count) of a scan row"""
    m = re.search(r'fused_head_multi_tuple_kernelILi(\d+)ELb([01])EE', row[0])
    if m:
        return ('count' if m.group(2) == '1' else 'hist', int(m.group(1)))
    return ('lut', int(re.search(r'fused_head_multi_lut_kernelILi(\d+)EE', row[0]).group(1)))


def test_every_instantiation_exists_once(scan):
    assert sorted(_key(r) for r in scan) == sorted((form, cm) for form in ('hist', 'count', 'lut') for cm in CLASS_STEPS)


def test_no_scratch_and_the_workgroup_fits(scan):
    for row in scan:
        kern, regs, scratch, waves = row
        assert scratch == 0 and waves >= WORKGROUP_WAVES, \
            '%s: %d registers, %d B scratch, %d waves' % (kern, regs, scratch, waves)


@pytest.mark.parametrize('form', ['hist', 'count', 'lut'])
def test_twelve_classes_hold_their_waves(scan, form):
    """equality: fewer waves is a regression, more means the comment above and DESIGN.md are out of date"""
    mine = [r for r in scan if _key(r) == (form, 12)]
    assert len(mine) == 1
    kern, regs, scratch, waves = mine[0]
    assert scratch == 0 and waves == PINNED_12[form], '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)
