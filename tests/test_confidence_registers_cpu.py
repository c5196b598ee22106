"""Register budget of the confidence kernels (csrc/confidence.hip) from tools/occupancy_scan.py, as
tests/test_calibration_registers_cpu.py holds the calibration kernels': every instantiation exists once, none has scratch (the
winner's score is picked by a chain of selects: an indexed read would put the class scores into scratch memory), and at 12
classes every mode holds at least the waves per SIMD that file pins for the calibration kernel of the same mode -- the fused
kernel runs the same statements without the LDS counting."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

CLASS_STEPS = [4, 8, 12, 16, 20, 24, 28, 32]
MODES = [0, 1, 2]                                       # Bayes, Dirichlet, mean
# waves per SIMD the calibration kernels are pinned to at 12 classes (tests/test_calibration_registers_cpu.py); the scan
# reports 5, 6 and 7 for the confidence head (registers: 89, 73, 65) and 8 for the kernel on materialised maps (30)
CALIBRATION_PINNED_12 = {0: 5, 1: 4, 2: 5}
CALIBRATION_PINNED_12_TABLE = 7
# a 256-thread workgroup is one wave per SIMD
WORKGROUP_WAVES = 1


@pytest.fixture(scope='module')
def scan():
    import occupancy_scan
    return occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'confidence.hip'))


def _fused_key(row):
    return tuple(int(v) for v in re.search(r'fused_head_multi_confidence_kernelILi(\d+)ELi(\d)EE', row[0]).groups())


def _map_key(row):
    return int(re.search(r'confidence_map_kernelILi(\d+)EE', row[0]).group(1))


def test_every_instantiation_exists_once(scan):
    fused = [r for r in scan if 'fused_head_multi_confidence_kernel' in r[0]]
    maps = [r for r in scan if 'confidence_map_kernel' in r[0]]
    assert sorted(_fused_key(r) for r in fused) == sorted((cm, mode) for cm in CLASS_STEPS for mode in MODES)
    assert sorted(_map_key(r) for r in maps) == CLASS_STEPS
    assert len(scan) == len(fused) + len(maps)


def test_no_scratch_anywhere(scan):
    for kern, regs, scratch, waves in scan:
        assert scratch == 0 and waves >= WORKGROUP_WAVES, '%s: %d registers, %d B scratch, %d waves' % (kern, regs, scratch, waves)


def test_the_calibration_pins_are_the_ones_this_file_restates():
    import test_calibration_registers_cpu as pinned
    assert pinned.PINNED_12 == CALIBRATION_PINNED_12 and pinned.PINNED_12_TABLE == CALIBRATION_PINNED_12_TABLE


@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
def test_twelve_classes_hold_the_waves_of_the_calibration_kernel(scan, mode):
    mine = [r for r in scan if 'fused_head_multi_confidence_kernel' in r[0] and _fused_key(r) == (12, mode)]
    assert len(mine) == 1
    kern, regs, scratch, waves = mine[0]
    assert scratch == 0 and waves >= CALIBRATION_PINNED_12[mode], '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)


def test_the_materialised_kernel_at_twelve_classes(scan):
    kern, regs, scratch, waves = [r for r in scan if 'confidence_map_kernel' in r[0] and _map_key(r) == 12][0]
    assert scratch == 0 and waves >= CALIBRATION_PINNED_12_TABLE, '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)
