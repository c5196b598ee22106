"""Register budgets of the MC-dropout (variance fusion) kernels (tools/occupancy_scan.py): the variance head recomputes every
sample's probabilities instead of holding T x C of them, so at 12 classes it must stay in registers at four waves per SIMD; the
sample replication is a streaming copy.  hipcc cross-compiles for gfx950 without a GPU."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

# (file, mangled-name fragment, fewest waves per SIMD, most scratch bytes)
BUDGETS = [
    ('heads.hip', 'variance_head_kernelILi12E', 4, 0),
    ('pointwise.hip', 'dropout_samples_kernel', 4, 0),
    ('fusion.hip', 'variance_fuse_kernelILi16E', 4, 0),
]


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_register_budgets_of_the_variance_kernels():
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
