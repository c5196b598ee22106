"""Register budgets of the MC-dropout Bayesian FCN kernels (tools/occupancy_scan.py) and the ABI bookkeeping of the new entry
points.  The uncertainty head keeps the first sample, two moment rows and the current sample in registers -- the rows of
variance_head_kernel (111 registers at 12 classes, four waves per SIMD) plus C logarithms per sample -- so it is held to the
same four waves; nothing may spill.  hipcc cross-compiles for gfx950 without a GPU."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

# (file, mangled-name fragment, fewest waves per SIMD, most scratch bytes)
BUDGETS = [
    ('heads.hip', 'mc_uncertainty_head_kernelILi12E', 4, 0),
    ('heads.hip', 'mc_uncertainty_head_kernelILi16E', 4, 0),
    ('heads.hip', 'mc_uncertainty_head_kernelILi', 1, 0),            # every instantiation the variance head has: no scratch
    ('pointwise.hip', 'dropout_samples_kernel', 4, 0),
    ('fusion.hip', 'sampling_uncertainty_kernelILi16E', 4, 0),
    ('fusion.hip', 'sampling_uncertainty_kernelILi32E', 1, 0),
]

NEW_ENTRY_POINTS = {       # name -> number of arguments
    'xv_dropout_samples_only': 7,
    'xv_dropout_samples_only_inplace': 6,
    'xv_mc_uncertainty_head_fwd': 13,
    'xv_sampling_uncertainty': 10,
}


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_register_budgets_of_the_uncertainty_kernels():
    import occupancy_scan
    csrc = occupancy_scan.CSRC
    files = sorted({f for f, _, _, _ in BUDGETS})
    table = occupancy_scan.scan([os.path.join(csrc, f) for f in files], workers=len(files))
    for fname, frag, min_waves, max_scratch in BUDGETS:
        rows = [r for r in table[fname] if frag in r[0]]
        assert rows, 'no kernel matching %s in %s' % (frag, fname)
        for kern, regs, scratch, waves in rows:
            assert waves >= min_waves and scratch <= max_scratch, \
                '%s: %d waves per SIMD (%d registers), %d B scratch; budget: >= %d waves, <= %d B' % (
                    kern, waves, regs, scratch, min_waves, max_scratch)
    heads = {r[0] for r in table['heads.hip'] if 'mc_uncertainty_head_kernelILi' in r[0]}
    assert len(heads) == 8, sorted(heads)                            # CM = 4, 8, .. 32, as variance_head_kernel


def test_new_entry_points_are_declared_listed_and_defined():
    from modular_semantic_segmentation_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'xview_hip.h')).read()
    csrc = os.path.join(ROOT, 'modular_semantic_segmentation_amd', 'csrc')
    sources = ''.join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith('.hip'))
    for name, nargs in NEW_ENTRY_POINTS.items():
        decl = re.search(r'\bint %s\(([^;{]*)\);' % name, header)
        assert decl, '%s is not declared in include/xview_hip.h' % name
        assert len(decl.group(1).split(',')) == nargs, name
        assert name in _lib.SIGNATURES, '%s is not in _lib.SIGNATURES' % name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        defn = re.search(r'extern "C" int %s\(([^{;]*)\)\s*\{' % name, sources)
        assert defn, '%s is not defined in csrc/' % name
        assert len(defn.group(1).split(',')) == nargs, name
    assert re.search(r'xv_version\(void\)\s*\{\s*return 604;', sources)
