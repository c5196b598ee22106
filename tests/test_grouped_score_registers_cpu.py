"""Register budget of the grouped scoring kernels (tools/occupancy_scan.py, as tests/test_kernel_registers_cpu.py pins their
ungrouped forms): the grouped joint histogram at 12 and 16 classes holds the four waves per SIMD of
fused_head_joint_hist_kernel<12 / 16>; the grouped confusion kernel is a 1 024-thread workgroup and must fit 128 registers;
no instantiation has scratch."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

CLASS_STEPS = [4, 8, 12, 16, 20]           # the entry point takes 2..20 classes: nothing is built beyond


@pytest.fixture(scope='module')
def rows():
    import occupancy_scan
    return occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'grouped_score.hip'))


def test_every_instantiation_exists_once(rows):
    hist = [r[0] for r in rows if 'fused_head_joint_hist_grouped_kernelILi' in r[0]]
    assert sorted(int(re.search(r'ILi(\d+)E', k).group(1)) for k in hist) == CLASS_STEPS
    assert len([r for r in rows if 'confusion_grouped_kernel' in r[0]]) == 1
    assert len(rows) == len(CLASS_STEPS) + 1


@pytest.mark.parametrize('cm', [12, 16])
def test_joint_hist_holds_four_waves_without_scratch(rows, cm):
    mine = [r for r in rows if 'fused_head_joint_hist_grouped_kernelILi%dE' % cm in r[0]]
    assert len(mine) == 1, mine
    kern, regs, scratch, waves = mine[0]
    assert waves >= 4 and scratch == 0, '%s: %d waves per SIMD (%d registers), %d B scratch' % (kern, waves, regs, scratch)


def test_confusion_fits_a_sixteen_wave_workgroup(rows):
    kern, regs, scratch, waves = [r for r in rows if 'confusion_grouped_kernel' in r[0]][0]
    assert waves >= 4 and scratch == 0, '%s: %d waves per SIMD (%d registers), %d B scratch' % (kern, waves, regs, scratch)


def test_no_scratch_anywhere(rows):
    for kern, regs, scratch, waves in rows:
        assert scratch == 0 and waves >= 1, '%s: %d registers, %d B scratch' % (kern, regs, scratch)
