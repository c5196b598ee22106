"""Register budget of the on-device augmentation kernel (tools/occupancy_scan.py, as tests/test_kernel_registers_cpu.py pins
the others): the three resampling stages nest inside one another with five float64 channels each, so the kernel must hold
them at four waves per SIMD without scratch."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')


def test_augment_kernel_budget():
    import occupancy_scan
    rows = [r for r in occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'augment.hip'))
            if 'augment_batch_kernel' in r[0]]
    assert len(rows) == 1, rows
    kern, regs, scratch, waves = rows[0]
    assert waves >= 4 and scratch == 0, '%s: %d waves per SIMD (%d registers), %d B scratch' % (kern, waves, regs, scratch)


def test_scan_builds_the_file_as_the_makefile_does():
    """No fused multiply-add may form in this file: both builds pass the flag."""
    import occupancy_scan
    assert occupancy_scan.EXTRA['augment.hip'] == ['-ffp-contract=off']
    mk = open(os.path.join(occupancy_scan.CSRC, 'Makefile')).read()
    assert 'FLAGS_augment.hip := -ffp-contract=off' in mk and ' augment.hip' in mk.split('SRCS :=')[1].split('\n')[0]
