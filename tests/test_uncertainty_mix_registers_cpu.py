"""Register budgets of the uncertainty-weighted Dirichlet fusion kernels (tools/occupancy_scan.py), the ABI bookkeeping of
their entry points and the host logic of get_model('uncertainty_mix').  The fusion head takes C^2 + C lgamma per expert and
pixel; their call sites stay rolled, so the kernel must hold its class rows in registers without scratch.  The pixel dropout
is a streaming copy and the moments pass is variance_head_kernel's per-pixel work: both are held to the four waves per SIMD
their siblings hold.  hipcc cross-compiles for gfx950 without a GPU."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

# (file, mangled-name fragment, fewest waves per SIMD, most scratch bytes)
BUDGETS = [
    ('heads.hip', 'uncertainty_dirichlet_head_kernelILi12E', 5, 0),         # 83 registers
    ('heads.hip', 'uncertainty_dirichlet_head_kernelILi', 1, 0),            # every instantiation: no scratch
    ('heads.hip', 'uncertainty_moments_kernelILi12E', 4, 0),                # 84 registers (five waves)
    ('heads.hip', 'uncertainty_moments_kernelILi', 1, 0),
    ('pointwise.hip', 'pixel_dropout_kernel', 4, 0),                        # 11 registers
    ('fusion.hip', 'uncertainty_dirichlet_fuse_kernelILi12E', 5, 0),        # 84 registers
    ('fusion.hip', 'uncertainty_dirichlet_fuse_kernelILi', 1, 0),
    ('fusion.hip', 'uncertainty_weights_kernelILi', 4, 0),
]
INSTANCES = {'uncertainty_dirichlet_head_kernelILi': 8, 'uncertainty_moments_kernelILi': 8,       # CM = 4, 8, .. 32
             'uncertainty_dirichlet_fuse_kernelILi': 8}

NEW_ENTRY_POINTS = {       # name -> number of arguments
    'xv_dropout_pixels_samples': 12,
    'xv_uncertainty_moments': 12,
    'xv_uncertainty_dirichlet_head_fwd': 17,
    'xv_uncertainty_dirichlet_fuse': 10,
    'xv_uncertainty_weights': 6,
}


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_register_budgets_of_the_uncertainty_mix_kernels():
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
    every = [r[0] for rows in table.values() for r in rows]
    for frag, count in INSTANCES.items():
        assert len({k for k in every if frag in k}) == count, frag


def test_uncertainty_mix_entry_points_are_declared_listed_and_defined():
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
    for name in ('dropout_pixels', 'dropout_pixels_samples', 'uncertainty_moments', 'uncertainty_dirichlet_head',
                 'uncertainty_dirichlet_fuse', 'uncertainty_weights'):
        from modular_semantic_segmentation_amd import ops
        assert callable(getattr(ops, name)), name


C = 12
DESC = ({'rgb': 'float32', 'depth': 'float32', 'labels': 'int32'},
        {'rgb': (None, None, 3), 'depth': (None, None, 1), 'labels': (None, None)}, C)
CFG = dict(modalities=['rgb', 'depth'], num_channels={'rgb': 3, 'depth': 1}, num_units=64, expert_model='fcn',
           class_prior='uniform', delta=1e-2, beta=1e-2, dropout_rate=0.5, num_samples=5)


def test_uncertainty_mix_registry_and_constructor_errors():
    from modular_semantic_segmentation_amd import get_model
    from modular_semantic_segmentation_amd.dirichlet_mix import DirichletFusion
    from modular_semantic_segmentation_amd.uncertainty_dirichlet_mix import UncertaintyMix, dirichlet_uncertainty_fusion
    assert get_model('uncertainty_mix') is UncertaintyMix and get_model('uncertainty_fusion') is UncertaintyMix
    assert issubclass(UncertaintyMix, DirichletFusion) and callable(dirichlet_uncertainty_fusion)
    # every refusal comes before anything touches a device
    for missing in ('dropout_rate', 'num_samples'):
        cfg = {k: v for k, v in CFG.items() if k != missing}
        with pytest.raises(UserWarning):
            UncertaintyMix(data_description=DESC, **cfg)
    with pytest.raises(ValueError):
        UncertaintyMix(data_description=DESC, **dict(CFG, num_samples=1))
    with pytest.raises(ValueError):
        UncertaintyMix(data_description=DESC, **dict(CFG, dropout_rate=0.0))
    with pytest.raises(UserWarning):
        UncertaintyMix(data_description=DESC, **dict(CFG, expert_model='adapnet'))


def test_uncertainty_mix_predict_before_fit_raises():
    """Without dirichlet_params the model builds (as DirichletFusion does) and refuses to predict until fit() has run; with
    them the tables are there.  The experts are left out: this runs without a GPU."""
    from modular_semantic_segmentation_amd.uncertainty_dirichlet_mix import UncertaintyMix

    class NoExperts(UncertaintyMix):
        def _build_experts(self):
            self.experts = {}

    data = {'rgb': np.zeros((1, 16, 16, 3), np.float32), 'depth': np.zeros((1, 16, 16, 1), np.float32)}
    net = NoExperts(data_description=DESC, device='cpu', **CFG)
    assert net.prediction == 0 and not net._graph_capturable()
    with pytest.raises(UserWarning):
        net.predict(data)
    params = {'rgb': np.ones((C, C)) + np.eye(C), 'depth': np.ones((C, C)) + 3 * np.eye(C), 'class_counts': np.arange(1, C + 1)}
    fitted = NoExperts(data_description=DESC, device='cpu', dirichlet_params=params, seed=7, **CFG)
    assert tuple(fitted.params_dev.shape) == (2, C, C) and fitted.params_dev.dtype.is_floating_point
    assert np.allclose(fitted.logprior.numpy(), np.log(1.0 / 14), atol=1e-6)            # the uniform prior of dirichlet_mix
    assert fitted._dropout_seed == 7 and 'sigma' not in fitted.config
    with pytest.raises(UserWarning):
        fitted.predict(data, output_attr='entropy')                                  # not an output of this model
