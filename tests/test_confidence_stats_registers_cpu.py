"""Register budget of the confidence statistics kernels (csrc/confidence_stats.hip) from tools/occupancy_scan.py, as
tests/test_confidence_registers_cpu.py holds the confidence kernels': every instantiation exists once, none has scratch (the
winner's and the label's score are picked by chains of selects), every one holds the two waves per SIMD of its 512-thread
workgroup, and at 12 classes every mode holds at least the waves per SIMD tests/test_calibration_registers_cpu.py pins for the
calibration kernel of the same mode -- these are the same statements plus the LDS counting."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

CLASS_STEPS = [4, 8, 12, 16, 20, 24, 28, 32]
MODES = [0, 1, 2]                                       # Bayes, Dirichlet, mean
# a 512-thread workgroup is two waves per SIMD: the least any instantiation may hold
WORKGROUP_WAVES = 2


@pytest.fixture(scope='module')
def scan():
    import occupancy_scan
    return occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'confidence_stats.hip'))


def _fused_key(row):
    return tuple(int(v) for v in re.search(r'fused_head_multi_confidence_stats_kernelILi(\d+)ELi(\d)EE', row[0]).groups())


def _map_key(row):
    return int(re.search(r'\d+confidence_stats_kernelILi(\d+)EE', row[0]).group(1))


def _is_fused(row):
    return 'fused_head_multi_confidence_stats_kernel' in row[0]


def test_every_instantiation_exists_once(scan):
    fused = [r for r in scan if _is_fused(r)]
    maps = [r for r in scan if not _is_fused(r) and 'confidence_stats_kernel' in r[0]]
    assert sorted(_fused_key(r) for r in fused) == sorted((cm, mode) for cm in CLASS_STEPS for mode in MODES)
    assert sorted(_map_key(r) for r in maps) == CLASS_STEPS
    assert len(scan) == len(fused) + len(maps)


def test_no_scratch_anywhere(scan):
    for kern, regs, scratch, waves in scan:
        assert scratch == 0 and waves >= WORKGROUP_WAVES, '%s: %d registers, %d B scratch, %d waves' % (kern, regs, scratch, waves)


@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
def test_twelve_classes_hold_the_waves_of_the_calibration_kernel(scan, mode):
    import test_calibration_registers_cpu as pinned
    mine = [r for r in scan if _is_fused(r) and _fused_key(r) == (12, mode)]
    assert len(mine) == 1
    kern, regs, scratch, waves = mine[0]
    assert scratch == 0 and waves >= pinned.PINNED_12[mode], '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)


def test_the_materialised_kernel_at_twelve_classes(scan):
    import test_calibration_registers_cpu as pinned
    kern, regs, scratch, waves = [r for r in scan if not _is_fused(r) and _map_key(r) == 12][0]
    assert scratch == 0 and waves >= pinned.PINNED_12_TABLE, '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)
