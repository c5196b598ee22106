"""Host side of the one-pass fusion comparison (fusion_comparison.py): the experts' matrices as marginals of the joint
histogram, the Dirichlet fit shared with DirichletFusion, and the two entry points of the fused average head in the ABI."""
import os

import numpy as np

C = 12


def test_marginals_of_a_joint_histogram_are_the_experts_matrices():
    from modular_semantic_segmentation_amd.fusion_comparison import expert_matrices_from_joint_hist
    rng = np.random.default_rng(3)
    n = 5000
    label, a, b = (rng.integers(0, C, n) for _ in range(3))
    hist = np.zeros((C, C, C), np.int64)
    np.add.at(hist, (label, a, b), 1)
    cm_a, cm_b = expert_matrices_from_joint_hist(hist)
    ref_a, ref_b = np.zeros((C, C), np.int64), np.zeros((C, C), np.int64)
    np.add.at(ref_a, (label, a), 1)
    np.add.at(ref_b, (label, b), 1)
    assert np.array_equal(cm_a, ref_a) and np.array_equal(cm_b, ref_b)
    assert not np.array_equal(cm_a, cm_b) and cm_a.sum() == n


def _statistics(golden_dir):
    """Sufficient statistics of two experts whose probabilities follow the confusion matrices of the notebook fixture: per
    ground-truth class the oracle's statistics of samples drawn around that class's row."""
    from oracle import fusion_oracle as fu
    g = np.load(os.path.join(golden_dir, 'notebook_868.npz'))
    rng = np.random.default_rng(7)
    labels = rng.integers(-1, C, (2, 24, 32))
    stats = {}
    for m in ('rgb', 'depth'):
        rows = g['cm_' + m].astype(np.float64) + 1.0
        alpha = 12.0 * rows / rows.sum(1, keepdims=True) + 0.2
        p = np.stack([rng.dirichlet(alpha[max(l, 0)]) for l in labels.ravel()]).reshape(labels.shape + (C,)).astype(np.float32)
        stats[m], counts = fu.sufficient_statistics(p, labels, C)
    return stats, counts


def _fit_as_before_the_move(counts, class_counts, delta, beta, modalities):
    """DirichletFusion._dirichlet_em as it stood before its body moved to dirichlet_mix.fit_dirichlet_params"""
    from modular_semantic_segmentation_amd.dirichlet_fit import find_dirichlet_priors

    def dirichlet_em(measurements):
        params = np.ones((C, C)).astype('float64')
        for c in range(C):
            if class_counts[c] == 0:
                params[:, c] = np.ones(C)
                continue
            ss = (measurements[c, :] / class_counts[c]).astype('float64')
            neg_ss = (measurements.sum(0) - measurements[c, :]) / (class_counts.sum() - class_counts[c])
            params[:, c] = find_dirichlet_priors(ss, neg_ss, np.ones(C, 'float64'), max_iter=10000, delta=delta, beta=beta)
        return params
    return {m: dirichlet_em(counts[m]) for m in modalities}


def test_moved_dirichlet_fit_returns_what_the_method_returned(golden_dir):
    from modular_semantic_segmentation_amd.dirichlet_mix import DirichletFusion, fit_dirichlet_params
    stats, counts = _statistics(golden_dir)
    counts = counts.copy()
    stats = {m: s.copy() for m, s in stats.items()}
    counts[5] = 0                                   # a class without samples keeps its all-ones column
    mods = ['rgb', 'depth']
    ref = _fit_as_before_the_move(stats, counts, 1e-2, 1e-2, mods)
    got = fit_dirichlet_params(stats, counts, 1e-2, 1e-2, C, mods)

    class Stub(object):
        config = {'num_classes': C}
        modalities = mods
    method = DirichletFusion._dirichlet_em(Stub(), stats, counts, 1e-2, 1e-2)
    for m in mods:
        assert got[m].dtype == np.float64 and got[m].shape == (C, C)
        assert np.array_equal(got[m], ref[m]) and np.array_equal(method[m], ref[m])
        assert np.array_equal(got[m][:, 5], np.ones(C)) and np.abs(got[m] - 1.0).max() > 0.1
    assert not np.array_equal(got['rgb'], got['depth'])
    other = fit_dirichlet_params(stats, counts, 1e-1, 1e-2, C, mods)
    assert not np.array_equal(other['rgb'], got['rgb'])                  # delta reaches the fit


def test_abi_declares_the_average_heads():
    from ctypes import c_int, c_void_p
    from modular_semantic_segmentation_amd import _lib, ops
    head = [c_void_p] * 4 + [c_int] * 4
    assert _lib.SIGNATURES['xv_fused_head_average_fwd'] == (c_int, head + [c_void_p, c_void_p])
    assert _lib.SIGNATURES['xv_fused_head_average_count_fwd'] == (c_int, head + [c_void_p, c_void_p, c_int, c_void_p])
    assert callable(ops.fused_head_average) and callable(ops.fused_head_average_count)
    src = open(os.path.join(_lib.CSRC, 'heads.hip')).read()
    for name in ('xv_fused_head_average_fwd', 'xv_fused_head_average_count_fwd'):
        assert src.count('extern "C" int %s(' % name) == 1
