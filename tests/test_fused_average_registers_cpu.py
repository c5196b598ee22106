"""Register budget of the fused average head (tools/occupancy_scan.py, as tests/test_kernel_registers_cpu.py pins its
siblings): the label and the counting form at 12 and 16 classes hold the four waves per SIMD of fused_head_kernel<12, 0> and
fused_head_joint_hist_kernel<12 / 16> without scratch; every other instantiation has no scratch."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

CLASS_STEPS = [4, 8, 12, 16, 20, 24, 28, 32]


@pytest.fixture(scope='module')
def rows():
    import occupancy_scan
    return [r for r in occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'heads.hip'))
            if 'fused_head_average_kernel' in r[0]]


def test_every_instantiation_exists_once(rows):
    """<CM, COUNT, FULL>: eight class steps, both forms, the run-time and the full class count"""
    keys = sorted(tuple(int(v) for v in re.search(r'ILi(\d+)ELb(\d)ELb(\d)E', r[0]).groups()) for r in rows)
    assert keys == sorted((cm, count, full) for cm in CLASS_STEPS for count in (0, 1) for full in (0, 1))


@pytest.mark.parametrize('cm', [12, 16])
@pytest.mark.parametrize('count', [0, 1], ids=['label', 'count'])
def test_four_waves_without_scratch(rows, cm, count):
    mine = [r for r in rows if 'ILi%dELb%dE' % (cm, count) in r[0]]
    assert len(mine) == 2, mine
    for kern, regs, scratch, waves in mine:
        assert waves >= 4 and scratch == 0, '%s: %d waves per SIMD (%d registers), %d B scratch' % (kern, waves, regs, scratch)


def test_no_scratch_anywhere(rows):
    for kern, regs, scratch, waves in rows:
        assert scratch == 0 and waves >= 1, '%s: %d registers, %d B scratch' % (kern, regs, scratch)
