"""Register budget of the counting head for two to four experts (fused_head_multi_count_kernel, csrc/multi_count.hip) from
tools/occupancy_scan.py: every instantiation exists once, none has scratch, and at 12 classes each holds the waves per SIMD
pinned here, next to the floors of its siblings fused_head_grid_score_kernel<12> and fused_head_multi_kernel<12, MODE, *>.
The launch's LDS (40 KB) lets four workgroups share a CU, so four waves per SIMD are all a launch can use: only the Dirichlet
form for four experts sits below that, by the four experts' log-probabilities it holds."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

CLASS_STEPS = [4, 8, 12, 16, 20, 24, 28, 32]
FORMS = [(0, 0), (2, 0), (1, 2), (1, 3), (1, 4)]        # (MODE, EU): Bayes and mean rolled over the experts, Dirichlet per count
# waves per SIMD at 12 classes as the scan reports them (registers: 95, 92, 92, 124, 160)
FLOORS_12 = {(0, 0): 5, (2, 0): 5, (1, 2): 5, (1, 3): 4, (1, 4): 3}
# the siblings' floors at 12 classes: what their amdgpu_waves_per_eu holds them to
SIBLING_FLOORS_12 = {r'fused_head_grid_score_kernelILi12EE': 4, r'fused_head_multi_kernelILi12ELi0ELb[01]E': 4,
                     r'fused_head_multi_kernelILi12ELi1ELb0E': 7, r'fused_head_multi_kernelILi12ELi1ELb1E': 8,
                     r'fused_head_multi_kernelILi12ELi2ELb[01]E': 4}


@pytest.fixture(scope='module')
def rows():
    import occupancy_scan
    scan = occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'multi_count.hip'))
    return [r for r in scan if 'fused_head_multi_count_kernel' in r[0]]


def _key(row):
    return tuple(int(v) for v in re.search(r'ILi(\d+)ELi(\d)ELi(\d)E', row[0]).groups())


def test_every_instantiation_exists_once(rows):
    assert sorted(_key(r) for r in rows) == sorted((cm, mode, eu) for cm in CLASS_STEPS for mode, eu in FORMS)


def test_no_scratch_anywhere(rows):
    for kern, regs, scratch, waves in rows:
        assert scratch == 0 and waves >= 1, '%s: %d registers, %d B scratch' % (kern, regs, scratch)


@pytest.mark.parametrize('form', FORMS, ids=['bayes', 'mean', 'dirichlet2', 'dirichlet3', 'dirichlet4'])
def test_twelve_classes_hold_their_waves(rows, form):
    mine = [r for r in rows if _key(r) == (12,) + form]
    assert len(mine) == 1
    kern, regs, scratch, waves = mine[0]
    assert scratch == 0 and waves >= FLOORS_12[form], '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)


def test_siblings_hold_their_floors():
    import occupancy_scan
    scan = occupancy_scan.scan_file(os.path.join(occupancy_scan.CSRC, 'heads.hip'))
    for pattern, floor in SIBLING_FLOORS_12.items():
        found = [r for r in scan if re.search(pattern, r[0])]
        assert found, pattern
        for kern, regs, scratch, waves in found:
            assert scratch == 0 and waves >= floor, '%s: %d waves per SIMD (%d registers)' % (kern, waves, regs)
