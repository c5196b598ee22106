"""Register budgets of every kernel the project pins (tools/occupancy_scan.py), in one table.  The compiler keeps a
loop-invariant LDS table in registers (one wave per SIMD) or requests every load of an unrolled body up front (412 registers):
a regression shows here before it shows as a slow kernel.  hipcc cross-compiles for gfx950 without a GPU; each source file the
table names is compiled to assembly once per run.  A new kernel with a budget gets a row here, under a heading of its feature."""
import os
import re
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')

# (file, mangled-name fragment, fewest waves per SIMD, most scratch bytes); every kernel the fragment matches is held to the row
BUDGETS = [
    # ---- heads, fusion and convolutions whose first compilations went wrong in round 5
    ('backward.hip', 'head_loss_kernelILi12ELb1E', 2, 0),                  # 253 registers; 412 before the taps were loaded once
    ('backward.hip', 'count_valid_kernel', 4, 0),
    ('heads.hip', 'fused_dirichlet_head_pk_kernelILi12ELi4E', 3, 0),       # 162 registers
    ('heads.hip', 'fused_head_kernelILi12ELi0ELb1ELi4E', 4, 0),            # Bayes: 98 registers (168 with per-pixel class sums)
    ('heads.hip', 'decoder_head_label4_kernelILi12E', 5, 0),
    ('fusion.hip', 'dirichlet_fuse_pk_kernelILi12E', 6, 0),                # 66 registers; 372 inside a grid-stride loop
    # round 6: the fused first pair carried 32 bytes of scratch in its RGB forms -- the masked tap gather of its edge-tile path
    # selected between array elements, which the compiler turned into an indexed load from a stack copy of the array
    ('conv_first_fused.hip', 'conv_first_pair_kernelILi3ELb0E', 2, 0),
    ('conv_first_fused.hip', 'conv_first_pair_kernelILi3ELb1E', 2, 0),
    ('conv_first_fused.hip', 'conv_first_pair_kernelILi1ELb0E', 2, 0),
    ('conv_wgrad.hip', 'conv_wgrad_lw_kernel', 2, 0),                      # 248 registers: 144 accumulators + the fragment rings
    # (36 bytes of true spills at the 128 registers a 1 024-thread workgroup allows: nine 64-bit load addresses per column
    # batch; a 60 us kernel)
    ('backward.hip', 'head_bwd_lowres_kernelILi12E', 4, 36),
    # round 6: the flat 1x1 filter gradient (all three forms) and the wide flat GEMM with its gathering modes: two 8-wave
    # workgroups' worth of registers (<= 128), no scratch
    ('conv_wgrad.hip', 'conv_wgrad_1x1_gemm_kernel', 4, 0),
    ('conv1x1_gemm.hip', 'conv1x1_gemm_wide_kernel', 4, 0),

    # ---- MC-dropout variance fusion: the variance head recomputes every sample's probabilities instead of holding T x C of
    # them, so at 12 classes it must stay in registers at four waves per SIMD; the sample replication is a streaming copy
    ('heads.hip', 'variance_head_kernelILi12E', 4, 0),
    ('pointwise.hip', 'dropout_samples_kernel', 4, 0),                     # (the Bayesian FCN pinned the same row)
    ('fusion.hip', 'variance_fuse_kernelILi16E', 4, 0),

    # ---- MC-dropout Bayesian FCN: the uncertainty head keeps the first sample, two moment rows and the current sample in
    # registers -- the rows of variance_head_kernel (111 registers at 12 classes, four waves per SIMD) plus C logarithms per
    # sample -- so it is held to the same four waves; nothing may spill
    ('heads.hip', 'mc_uncertainty_head_kernelILi12E', 4, 0),
    ('heads.hip', 'mc_uncertainty_head_kernelILi16E', 4, 0),
    ('heads.hip', 'mc_uncertainty_head_kernelILi', 1, 0),            # every instantiation the variance head has: no scratch
    ('fusion.hip', 'sampling_uncertainty_kernelILi16E', 4, 0),
    ('fusion.hip', 'sampling_uncertainty_kernelILi32E', 1, 0),

    # ---- uncertainty-weighted Dirichlet fusion: the fusion head takes C^2 + C lgamma per expert and pixel; their call sites
    # stay rolled, so the kernel must hold its class rows in registers without scratch.  The pixel dropout is a streaming copy
    # and the moments pass is variance_head_kernel's per-pixel work: both are held to the four waves their siblings hold
    ('heads.hip', 'uncertainty_dirichlet_head_kernelILi12E', 5, 0),         # 83 registers
    ('heads.hip', 'uncertainty_dirichlet_head_kernelILi', 1, 0),            # every instantiation: no scratch
    ('heads.hip', 'uncertainty_moments_kernelILi12E', 4, 0),                # 84 registers (five waves)
    ('heads.hip', 'uncertainty_moments_kernelILi', 1, 0),
    ('pointwise.hip', 'pixel_dropout_kernel', 4, 0),                        # 11 registers
    ('fusion.hip', 'uncertainty_dirichlet_fuse_kernelILi12E', 5, 0),        # 84 registers
    ('fusion.hip', 'uncertainty_dirichlet_fuse_kernelILi', 1, 0),
    ('fusion.hip', 'uncertainty_weights_kernelILi', 4, 0),

    # ---- uncertainty benchmarks: the scoring head holds mc_uncertainty_head_kernel's budget
    ('heads.hip', 'mc_uncertainty_score_kernelILi12E', 4, 0),
    ('heads.hip', 'mc_uncertainty_score_kernelILi16E', 4, 0),
    ('heads.hip', 'mc_uncertainty_score_kernelILi', 1, 0),
    ('fusion.hip', 'uncertainty_stats_kernel', 4, 0),

    # ---- fusion grid search: the budget mc_uncertainty_score_kernel holds
    ('heads.hip', 'fused_head_grid_score_kernelILi12E', 4, 0),
    ('heads.hip', 'fused_head_grid_score_kernelILi16E', 4, 0),
    ('heads.hip', 'fused_head_grid_score_kernelILi', 1, 0),
    ('heads.hip', 'fused_head_joint_hist_kernelILi12E', 4, 0),
    ('heads.hip', 'fused_head_joint_hist_kernelILi16E', 4, 0),
    ('heads.hip', 'fused_head_joint_hist_kernelILi', 1, 0),
]

# mangled-name fragment -> the first template argument (classes rounded up to 4) of its instantiations, over every scanned file
CLASS_STEPS = [4, 8, 12, 16, 20, 24, 28, 32]
INSTANCES = {
    'mc_uncertainty_head_kernelILi': CLASS_STEPS,                # as variance_head_kernel
    'uncertainty_dirichlet_head_kernelILi': CLASS_STEPS,
    'uncertainty_moments_kernelILi': CLASS_STEPS,
    'uncertainty_dirichlet_fuse_kernelILi': CLASS_STEPS,
    'mc_uncertainty_score_kernelILi': CLASS_STEPS,
    'fused_head_grid_score_kernelILi': CLASS_STEPS,
    'fused_head_joint_hist_kernelILi': CLASS_STEPS,
}


@pytest.fixture(scope='module')
def table():
    """{file: [(kernel, registers, scratch bytes, waves per SIMD)]} of the files BUDGETS names, each compiled once"""
    import occupancy_scan
    files = sorted({row[0] for row in BUDGETS})
    return occupancy_scan.scan([os.path.join(occupancy_scan.CSRC, f) for f in files], workers=min(len(files), 16))


@pytest.mark.parametrize('fname,frag,min_waves,max_scratch', BUDGETS, ids=[row[1] for row in BUDGETS])
def test_register_budget(table, fname, frag, min_waves, max_scratch):
    rows = [r for r in table[fname] if frag in r[0]]
    assert rows, 'no kernel matching %s in %s' % (frag, fname)
    for kern, regs, scratch, waves in rows:
        assert waves >= min_waves and scratch <= max_scratch, \
            '%s: %d waves per SIMD (%d registers), %d B scratch; budget: >= %d waves, <= %d B' % (
                kern, waves, regs, scratch, min_waves, max_scratch)


def test_budget_table_has_one_row_per_fragment():
    assert len({row[1] for row in BUDGETS}) == len(BUDGETS) == 39          # the fragment is the case's id


def test_instantiations(table):
    every = {r[0] for rows in table.values() for r in rows}
    for frag, steps in INSTANCES.items():
        kernels = {k for k in every if frag in k}
        assert len(kernels) == len(steps), (frag, sorted(kernels))
        assert sorted(int(re.search(r'ILi(\d+)E', k).group(1)) for k in kernels) == steps, frag
