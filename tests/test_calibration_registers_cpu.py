"""Register budget of the calibration kernels (csrc/calibration.hip) from tools/occupancy_scan.py, as
tests/test_agreement_registers_cpu.py holds the agreement kernels': every instantiation exists once, none has scratch (the
class scores of a pixel stay in registers while every temperature walks over them: an indexed read of s[label] would put them
into scratch memory), every one holds the two waves per SIMD of its 512-thread workgroup, and the 12-class forms hold the
waves the scan reports."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

CLASS_STEPS = [4, 8, 12, 16, 20, 24, 28, 32]
MODES = [0, 1, 2]                                       # Bayes, Dirichlet, mean
# waves per SIMD at 12 classes as the scan reports them (registers: 92, 98, 88; the kernel on materialised maps: 47)
PINNED_12 = {0: 5, 1: 4, 2: 5}
PINNED_12_TABLE = 7
# a 512-thread workgroup is two waves per SIMD: the least any instantiation may hold
WORKGROUP_WAVES = 2


@pytest.fixture(scope='module')
def scan():
    import occupancy_scan
    return occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'calibration.hip'))


def _fused_key(row):
    return tuple(int(v) for v in re.search(r'fused_head_multi_calibration_kernelILi(\d+)ELi(\d)EE', row[0]).groups())


def _table_key(row):
    return int(re.search(r'calibration_table_kernelILi(\d+)EE', row[0]).group(1))


def test_every_instantiation_exists_once(scan):
    fused = [r for r in scan if 'fused_head_multi_calibration_kernel' in r[0]]
    table = [r for r in scan if 'calibration_table_kernel' in r[0]]
    assert sorted(_fused_key(r) for r in fused) == sorted((cm, mode) for cm in CLASS_STEPS for mode in MODES)
    assert sorted(_table_key(r) for r in table) == CLASS_STEPS
    assert len(scan) == len(fused) + len(table)


def test_no_scratch_anywhere(scan):
    for kern, regs, scratch, waves in scan:
        assert scratch == 0 and waves >= WORKGROUP_WAVES, '%s: %d registers, %d B scratch, %d waves' % (kern, regs, scratch, waves)


@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
def test_twelve_classes_hold_their_waves(scan, mode):
    mine = [r for r in scan if 'fused_head_multi_calibration_kernel' in r[0] and _fused_key(r) == (12, mode)]
    assert len(mine) == 1
    kern, regs, scratch, waves = mine[0]
    assert scratch == 0 and waves >= PINNED_12[mode], '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)


def test_the_materialised_kernel_at_twelve_classes(scan):
    kern, regs, scratch, waves = [r for r in scan if 'calibration_table_kernel' in r[0] and _table_key(r) == 12][0]
    assert scratch == 0 and waves >= PINNED_12_TABLE, '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)
