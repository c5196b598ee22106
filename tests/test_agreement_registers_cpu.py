"""Register budget of the agreement kernels (csrc/agreement.hip) from tools/occupancy_scan.py, as
tests/test_multi_count_registers_cpu.py holds the counting head's: every instantiation exists once, none has scratch, and at 12
classes each form holds at least the waves per SIMD of its fused_head_multi_count_kernel sibling -- it carries strictly less
state: one parameter set, so the experts run in a rolled loop on running state in every mode and ONE instantiation serves two,
three and four experts where the counting head's Dirichlet form has one per expert count."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

CLASS_STEPS = [4, 8, 12, 16, 20, 24, 28, 32]
MODES = [0, 1, 2]                                       # Bayes, Dirichlet, mean
# waves per SIMD at 12 classes as the scan reports them (registers: 73, 72, 72)
PINNED_12 = {0: 6, 1: 7, 2: 7}
# the counting head's at 12 classes (tests/test_multi_count_registers_cpu.py): Bayes, mean, Dirichlet with 2 / 3 / 4 experts
SIBLING_12 = {0: [5], 2: [5], 1: [5, 4, 3]}
# a 512-thread workgroup is two waves per SIMD: the least any instantiation may hold
WORKGROUP_WAVES = 2


@pytest.fixture(scope='module')
def scan():
    import occupancy_scan
    return occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'agreement.hip'))


def _key(row):
    return tuple(int(v) for v in re.search(r'fused_head_multi_agreement_kernelILi(\d+)ELi(\d)EE', row[0]).groups())


def test_every_instantiation_exists_once(scan):
    fused = [r for r in scan if 'fused_head_multi_agreement_kernel' in r[0]]
    assert sorted(_key(r) for r in fused) == sorted((cm, mode) for cm in CLASS_STEPS for mode in MODES)
    assert len([r for r in scan if 'agreement_table_kernel' in r[0]]) == 1
    assert len(scan) == len(fused) + 1


def test_no_scratch_anywhere(scan):
    for kern, regs, scratch, waves in scan:
        assert scratch == 0 and waves >= WORKGROUP_WAVES, '%s: %d registers, %d B scratch, %d waves' % (kern, regs, scratch, waves)


@pytest.mark.parametrize('mode', MODES, ids=['bayes', 'dirichlet', 'mean'])
def test_twelve_classes_hold_their_siblings_waves(scan, mode):
    mine = [r for r in scan if 'fused_head_multi_agreement_kernel' in r[0] and _key(r) == (12, mode)]
    assert len(mine) == 1
    kern, regs, scratch, waves = mine[0]
    assert scratch == 0 and waves >= PINNED_12[mode], '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)
    assert PINNED_12[mode] >= max(SIBLING_12[mode])


def test_the_materialised_kernel_fills_the_simd(scan):
    kern, regs, scratch, waves = [r for r in scan if 'agreement_table_kernel' in r[0]][0]
    assert scratch == 0 and waves == 8, '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)
