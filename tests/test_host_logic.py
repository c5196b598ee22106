"""CPU-only tests: host logic of the product against the reference-generated golden vectors,
and the C-ABI library's exports (no compute calls without a GPU)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p

from modular_semantic_segmentation_amd import _lib, get_model
from modular_semantic_segmentation_amd import base_model, bayes_mix, custom_layers, dirichlet_fit, dirichlet_mix, fcn
from oracle import fusion_oracle as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def test_library_builds_and_exports_every_declared_symbol():
    _lib.build()
    header = open(os.path.join(ROOT, 'include', 'xview_hip.h')).read()
    declared = set(re.findall(r'\b(xv_[a-z0-9_]+)\s*\(', header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    handle = _lib.lib()
    for name in declared:
        assert hasattr(handle, name)
    assert handle.xv_version() >= 100
    assert handle.xv_arch() == b'gfx950'
    assert handle.xv_packed_weight_bytes(3, 64, 128) == 3 * 9 * 64 * 128 * 2     # three packed images (generations 1, 2, 4 / 5 on 16x16x32 blocks)
    assert handle.xv_packed_weight_bytes_f8(3, 128, 64) == 256 + 2 * 9 * 128 * 64    # header + generations 1 and 4
    assert handle.xv_packed_weight_bytes_f8(3, 64, 64) == 256 + 2 * 9 * 64 * 64     # 64-channel e4m3 chunks: generation 4 only
    assert handle.xv_packed_weight_bytes_f8(1, 64, 64) == 0                         # 1x1: 128-channel chunks
    assert handle.xv_packed_weight_bytes(1, 64, 128) == 64 * 128 * 2
    assert handle.xv_packed_weight_bytes(3, 3, 64) == 0          # first layer is not an MFMA conv


# Hand-written from the header, independent of the parser: one entry per rule of its type map
_ACT = POINTER(_lib.xv_act)
PINNED_SIGNATURES = {
    'xv_adam_step': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_float,
                             c_void_p]),
    'xv_dropout_samples': (c_int, [_ACT, _ACT, c_int, c_float, c_uint64, c_uint64, c_void_p]),
    'xv_bayes_fuse': (c_int, [POINTER(c_void_p), c_int, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    'xv_variance_fuse': (c_int, [POINTER(c_void_p), POINTER(c_void_p), c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    'xv_conv2d_fwd_ws': (c_int, [_ACT, c_void_p, c_void_p, _ACT, _ACT, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    'xv_source_hash': (c_char_p, []),
    'xv_packed_weight_bytes': (c_size_t, [c_int, c_int, c_int]),
    'xv_uncertainty_dirichlet_head_fwd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p]),
}
# the source file that has to hold the definition, for the entry points whose feature pinned it
DEFINED_IN = {'xv_uncertainty_stats': 'fusion.hip', 'xv_mc_uncertainty_score_fwd': 'heads.hip',
              'xv_fused_head_grid_score_fwd': 'heads.hip', 'xv_fused_head_grid_capacity': 'heads.hip',
              'xv_fused_head_joint_hist_fwd': 'heads.hip'}
OPS_WRAPPERS = ('dropout_pixels', 'dropout_pixels_samples', 'uncertainty_moments', 'uncertainty_dirichlet_head',
                'uncertainty_dirichlet_fuse', 'uncertainty_weights')


def _count(params):
    return 0 if params.strip() in ('', 'void') else len(params.split(','))


def test_abi_is_one_table_header_sources_and_ctypes():
    """Every symbol of include/xview_hip.h: in _lib.SIGNATURES (which is derived from the header), defined once in csrc/ with
    the declared number of parameters; the two ctypes structures against the header's members; the parser against
    hand-written expectations."""
    header = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(os.path.join(ROOT, 'include', 'xview_hip.h')).read(), flags=re.S)
    declared = {name: _count(params) for name, params in re.findall(r'\b(xv_\w+)\s*\(([^()]*)\)\s*;', header)}
    assert len(declared) >= 154 and set(declared) == set(_lib.SIGNATURES), set(declared) ^ set(_lib.SIGNATURES)

    csrc = os.path.join(ROOT, 'modular_semantic_segmentation_amd', 'csrc')
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith('.hip')}
    # Every source file reaches the header through xv_common.h, so the compiler itself refuses a definition whose types conflict
    # with its declaration (both are extern "C": same name, other parameters = "conflicting types"); what is left to check here
    # is that each declaration HAS a definition, once, and the parameter counts as a second line of defence.
    assert '#include "../../include/xview_hip.h"' in open(os.path.join(csrc, 'xv_common.h')).read()
    for fname, text in sources.items():
        assert '#include "xv_common.h"' in text, fname
    defined = {}
    for fname, text in sources.items():
        for name, params in re.findall(r'extern "C"\s+(?:const\s+)?\w+\s*\*?\s*(xv_\w+)\s*\(([^{;]*)\)\s*\{', text):
            defined.setdefault(name, []).append((fname, _count(params)))
    for name, nargs in declared.items():
        assert len(defined.get(name, [])) == 1, '%s: defined in %s' % (name, defined.get(name))
        fname, ndef = defined[name][0]
        assert ndef == nargs == len(_lib.SIGNATURES[name][1]), (name, ndef, nargs, len(_lib.SIGNATURES[name][1]))
        assert DEFINED_IN.get(name, fname) == fname, name
    assert len(re.findall(r'xv_version\(void\)\s*\{\s*return 604;', ''.join(sources.values()))) == 1
    # the plain uncertainty head and its entry point take no temperature (the scoring head does)
    assert 'inv_t' not in re.search(r'void mc_uncertainty_head_kernel\((.*?)\)\s*\{', sources['heads.hip'], re.S).group(1)
    from modular_semantic_segmentation_amd import ops
    for name in OPS_WRAPPERS:
        assert callable(getattr(ops, name)), name

    for name, expected in PINNED_SIGNATURES.items():
        assert _lib.SIGNATURES[name] == expected, name
    assert _lib.CONSTANTS == {'XV_OK': 0, 'XV_EINVAL': -1, 'XV_ESHAPE': -2, 'XV_EWORKSPACE': -3, 'XV_BF16': 0, 'XV_FP8': 1}
    assert (ops.BF16, ops.FP8, ops.XV_ESHAPE) == (0, 1, -2)

    # the hand-written structures: the header's members in order, by name, type and width
    assert sorted(_lib.STRUCTS) == ['xv_act', 'xv_pack_desc']
    for cls, size in ((_lib.xv_act, 32), (_lib.xv_pack_desc, 40)):
        members = _lib.STRUCTS[cls.__name__]
        assert [n for n, _ in cls._fields_] == [n for n, _ in members], cls.__name__
        for (field, ctype), (_, ctext) in zip(cls._fields_, members):
            want = c_void_p if ctext.endswith('*') else {'int32_t': c_int32}[ctext]
            assert ctype is want and ctypes.sizeof(ctype) == (8 if want is c_void_p else 4), (cls.__name__, field, ctext)
        assert ctypes.sizeof(cls) == size
    assert _lib.STRUCTS['xv_act'][0] == ('data', 'void*') and _lib.STRUCTS['xv_pack_desc'][0] == ('w_hwio', 'const float*')


def test_header_parser_on_synthetic_headers():
    for bad in ('int xv_f(double x, void* stream);', 'void xv_f(int n);', 'int xv_f(unsigned n);', 'int xv_f(float*** p);',
                'int xv_f(int);', 'int xv_f(int n); int xv_f(int n);', 'struct s;'):
        with pytest.raises(_lib.XvError, match='xview_hip.h'):
            _lib.parse_header(bad)
    with pytest.raises(_lib.XvError, match='xv_bad_one'):          # the message names the declaration
        _lib.parse_header('int xv_good(int n);\nint xv_bad_one(int n, long m);')
    text = '''
        #define XV_SEVEN (-7)     /* a code */
        #define XV_THREE 3        // another
        typedef struct xv_thing {
          const float* p;         /* a pointer */
          int32_t a, b;
        } xv_thing;
        /* int xv_commented_out(int n); */
        // int xv_commented_out_too(int n);
        int xv_multi(const float* a,   /* first */
                     int64_t n,        // count
                     const float* const* table,
                     /* a line of its own, with a ; and a , in it */
                     size_t bytes, float rate, uint64_t seed, const xv_act* y,
                     const xv_pack_desc* descs,
                     void* stream);
        size_t xv_none(void);
        const char* xv_name(void);
    '''
    functions, constants, structs = _lib.parse_header(text)
    assert functions == {
        'xv_multi': (c_int, [c_void_p, c_int64, POINTER(c_void_p), c_size_t, c_float, c_uint64, POINTER(_lib.xv_act), c_void_p,
                             c_void_p]),
        'xv_none': (c_size_t, []),
        'xv_name': (c_char_p, []),
    }
    assert constants == {'XV_SEVEN': -7, 'XV_THREE': 3}
    assert structs == {'xv_thing': [('p', 'const float*'), ('a', 'int32_t'), ('b', 'int32_t')]}


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, 'HEADER', str(tmp_path / 'nope.h'))
    with pytest.raises(_lib.XvError, match='nope.h'):
        _lib._read_header()


def test_abi_rejects_bad_arguments_without_touching_the_gpu():
    handle = _lib.lib()
    assert handle.xv_softmax_argmax(None, 10, 12, None, None, None) == -1           # XV_EINVAL
    assert handle.xv_bayes_fuse_lut(None, None, None, 12, 10, None, None) == -1
    a = _lib.xv_act(None, 1, 16, 16, 64)
    assert handle.xv_maxpool2x2_fwd(a, a, None) == -1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_lib.XvError):
        _lib.lib()


def test_bilinear_filter_golden(golden_dir):
    g = _g(golden_dir, 'bilinear_kernels.npz')
    np.testing.assert_array_equal(custom_layers.bilinear_filter([4, 4, 5, 5]), g['k4'].astype(np.float32))
    np.testing.assert_array_equal(custom_layers.bilinear_filter([16, 16, 3, 3]), g['k16'].astype(np.float32))
    assert custom_layers.is_bilinear_filter(g['k16'])
    bad = g['k4'].copy()
    bad[0, 0, 0, 1] = 0.1
    assert not custom_layers.is_bilinear_filter(bad)


def test_score_measures_golden(golden_dir):
    g = _g(golden_dir, 'notebook_868.npz')
    for who in ('rgb', 'depth', 'fusion'):
        m = base_model.score_measures(g['test_cm_' + who])
        for key in ('mean_IoU', 'mean_F1', 'total_accuracy'):
            assert m[key] == float(g['%s__%s' % (who, key)])
        for key in ('IoU', 'F1', 'precision', 'recall'):
            np.testing.assert_allclose(m[key], g['%s__%s' % (who, key)], rtol=0, atol=5e-9)


@pytest.mark.parametrize('name,prior', [('data', 'data'), ('uniform', 'uniform'), ('w0p5', 0.5)])
def test_bayes_decision_matrix_golden(golden_dir, name, prior):
    g = _g(golden_dir, 'notebook_868.npz')
    mats = [g['cm_rgb'].astype('float32').T, g['cm_depth'].astype('float32').T]
    lut = _g(golden_dir, 'bayes_lut.npz')['lut_' + name]
    np.testing.assert_array_equal(bayes_mix.bayes_decision_matrix(mats, prior), lut)


def test_bayes_tables_match_oracle(golden_dir):
    g = _g(golden_dir, 'notebook_868.npz')
    mats = [g['cm_rgb'].astype('float32').T, g['cm_depth'].astype('float32').T]
    mats[0][:, 3] = 0                                  # empty class -> nan_to_num path
    C = 12
    a, b = np.meshgrid(np.arange(C), np.arange(C), indexing='ij')
    for prior in ('data', 'uniform', 0.25):
        loglik, logprior = bayes_mix.bayes_tables(mats, prior)
        score = (loglik[0][a] + loglik[1][b]) + logprior
        ref, _, _ = fu.bayes_fusion([a, b], mats, prior)
        np.testing.assert_array_equal(score.astype(np.float32), ref)


def test_dirichlet_fitter_golden(golden_dir):
    f = _g(golden_dir, 'dirichlet_fit.npz')
    for i in range(int(f['num_cases'])):
        delta, beta = f['case%d_delta_beta' % i]
        ss = f['case%d_ss' % i]
        alpha = dirichlet_fit.find_dirichlet_priors(ss, f['case%d_neg_ss' % i], np.ones(len(ss)),
                                                    max_iter=10000, delta=delta, beta=beta)
        np.testing.assert_allclose(alpha, f['case%d_alpha' % i], rtol=1e-12, atol=1e-12)


def test_dirichlet_fitter_degenerate_golden(golden_dir):
    """Round 3: statistics at the corners -- a class seen on ONE pixel, experts certain of a class (log p = 0 / log 1e-10),
    statistics near 0, strong delta / beta, a far start cut off after 20 iterations, a fit that runs away until max_iter
    -- fitted by the IMPORTED reference (tests/golden/make_golden.py, dirichletDifferentiation.py:129-192).  The
    vectorised fitter takes the same branches (same terminating message) and agrees to rounding: the two accumulate
    the same sums in another order (Python loops vs numpy), 1e-9 relative after up to 10 000 iterations."""
    import contextlib
    import io
    from modular_semantic_segmentation_amd.dirichlet_fit import find_dirichlet_priors
    f = _g(golden_dir, 'dirichlet_fit_degenerate.npz')
    assert int(f['num_cases']) >= 8
    for i in range(int(f['num_cases'])):
        max_iter, delta, beta = f['case%d_params' % i]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            got = find_dirichlet_priors(f['case%d_ss' % i], f['case%d_neg_ss' % i], f['case%d_init' % i], max_iter=int(max_iter),
                                        delta=float(delta), beta=float(beta), verbose=True)
        want = f['case%d_alpha' % i]
        assert buf.getvalue().strip().splitlines()[-1] == str(f['case%d_message' % i]), (i, buf.getvalue())
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-12, err_msg='case %d' % i)
        assert np.all(got > 0)


def test_dirichlet_tables_match_oracle():
    rng = np.random.default_rng(0)
    C = 12
    A = [rng.uniform(0.3, 5, (C, C)).astype(np.float32) for _ in range(2)]
    counts = rng.integers(0, 100, C)
    p = [rng.dirichlet(np.ones(C), size=(1, 3, 4)).astype(np.float32) for _ in range(2)]
    for prior_cfg, sigma in (('data', 1.0), ('uniform', 0.7), (0.4, 1.5)):
        am1, lognorm, logprior = dirichlet_mix.dirichlet_tables(A, counts, prior_cfg, sigma)
        score = logprior.copy()[None, None, None, :]
        total = 0
        for e in range(2):
            lx = np.log(np.float32(1e-20) + fu.renormalise(p[e]))
            total = total + (lx @ am1[e].T - lognorm[e])
        ref = fu.dirichlet_fusion([fu.renormalise(q) for q in p], A, fu.dirichlet_prior(counts, prior_cfg), sigma)
        np.testing.assert_allclose(total + score, ref, rtol=1e-5, atol=1e-3)


def test_variable_schema_matches_reference_names(golden_dir):
    names = json.load(open(os.path.join(golden_dir, 'weight_names.json')))['variables']
    shapes = fcn.variable_shapes('rgb', 3, 64, 12)
    assert list(shapes) == names
    assert shapes['rgb/conv1_1/kernel'] == (3, 3, 3, 64)
    assert shapes['rgb/upscore/kernel'] == (16, 16, 64, 64)
    assert shapes['rgb/score/kernel'] == (1, 1, 64, 12)
    n_train = sum(int(np.prod(s)) for k, s in shapes.items() if 'upscore' not in k)
    assert n_train == 14781132
    bn = fcn.variable_shapes('rgb', 3, 64, 12, batch_normalization=True)
    assert bn['rgb/conv3_2/moving_variance'] == (256,)


def test_iterate_batches_dict_and_samples():
    data = {'rgb': np.zeros((5, 4, 4, 3), np.float32), 'labels': np.arange(5)}
    sizes = [len(b['labels']) for b in base_model.iterate_batches(data, 2)]
    assert sizes == [2, 2, 1]
    samples = ({'rgb': np.zeros((4, 4, 3)), 'labels': np.array(i)} for i in range(5))
    got = [b['labels'].tolist() for b in base_model.iterate_batches(samples, 3, max_batches=1)]
    assert got == [[0, 1, 2]]


class _HostOnly(base_model.BaseModel):
    """BaseModel without engines: exercises the npz import/export logic on the CPU."""

    def _build_graph(self):
        self.variables = {'rgb/conv1_1/kernel': np.zeros((3, 3, 3, 64), np.float32),
                          'rgb/conv1_1/bias': np.zeros(64, np.float32)}
        self.prediction = 'label'
        self.loss = None


def test_export_import_weights_roundtrip(tmp_path, capsys):
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, 12)
    with _HostOnly(desc, name='SimpleFCN', output_dir=str(tmp_path), device='cpu') as net:
        net.variables['rgb/conv1_1/bias'][:] = 3
        net.global_step = 7
        path = net.export_weights()
    assert os.path.basename(path) == 'SimpleFCN_weights_7.npz'
    saved = np.load(path)
    assert set(saved.keys()) == {'rgb/conv1_1/kernel', 'rgb/conv1_1/bias', 'global_step'}
    net2 = _HostOnly(desc, device='cpu')
    net2.import_weights(path, warnings=False)
    assert np.all(net2.variables['rgb/conv1_1/bias'] == 3)
    # legacy 'prefix_layer/...' names and prefix translation (base_model.py:435-437, 411-425)
    legacy = str(tmp_path / 'legacy.npz')
    np.savez(legacy, **{'depth_conv1_1/kernel': np.ones((3, 3, 3, 64), np.float32),
                        'depth_conv1_1/bias': np.full(64, 5, np.float32)})
    net2.import_weights(legacy, translate_prefix='rgb', warnings=False)
    assert np.all(net2.variables['rgb/conv1_1/bias'] == 5)
    # wrong shape (base_model.py:438-445, literally): reported and skipped outside chill mode; in chill mode the
    # reference attempts the assign anyway, which tf.assign rejects with a ValueError
    bad = str(tmp_path / 'bad.npz')
    np.savez(bad, **{'rgb/conv1_1/bias': np.zeros(3, np.float32)})
    net2.import_weights(bad, warnings=True)
    assert 'wrong shape found for rgb/conv1_1/bias' in capsys.readouterr().out
    assert np.all(net2.variables['rgb/conv1_1/bias'] == 5)
    with pytest.raises(ValueError):
        net2.import_weights(bad, chill_mode=True, warnings=False)
    # global_step is a global variable of a trainable model: restored on import (base_model.py:153-156,430)
    assert net2.global_step == 7


def test_captured_graph_is_dropped_when_variables_change():
    """A hipGraph captured by `capture_graph` replays raw weight pointers; every path that replaces the weights
    must drop it (the engines allocate new tensors in `load`)."""
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, 12)
    net = _HostOnly(desc, device='cpu')
    net._graph = ('graph', {}, None, {})
    net._variables_changed()
    assert net._graph is None
    net._graph = ('graph', {}, None, {})
    net._initialize_graph()
    assert net._graph is None


def test_registry_names():
    assert get_model('fcn').__name__ == 'SimpleFCN'
    assert get_model('bayes_mix') is get_model('bayes_fusion')
    assert get_model('dirichlet_fusion').__name__ == 'DirichletFusion'
    assert get_model('average_mix').__name__ == 'AverageFusion'
    with pytest.raises(UserWarning):
        get_model('nope')


def test_fusion_fcn_variable_schema():
    """Variable names of the joint baseline follow the reference graph: trunks '{prefix}_convX_Y' (vgg16.py:18-37),
    'fused_score_conv4/5', 'fused_upscore_conv5' (fusion_fcn.py:30-36), decoder scope 'fused' with batch norm."""
    from modular_semantic_segmentation_amd.fusion_fcn import variable_shapes
    from oracle import fcn_oracle as fo
    prefixes, nch = {'rgb': 'rgb', 'depth': 'depth'}, {'rgb': 3, 'depth': 1}
    shapes = variable_shapes(prefixes, nch, 64, 12)
    assert shapes['rgb_conv1_1/kernel'] == (3, 3, 3, 64) and shapes['depth_conv1_1/kernel'] == (3, 3, 1, 64)
    assert shapes['fused_score_conv4/kernel'] == (1, 1, 1024, 64)
    assert shapes['fused/upscore/kernel'] == (16, 16, 64, 64) and shapes['fused/score/gamma'] == (12,)
    ref = fo.init_fusion_fcn_weights(prefixes, nch, 64, 12)
    assert {k: tuple(v.shape) for k, v in ref.items()} == shapes


def test_split_test_data_is_the_sklearn_half_split():
    """experiments.split_test_data == train_test_split(test_size=.5, random_state=1) of the reference flow
    (experiments/bayes_fusion.py:21-33): deterministic, disjoint, covering."""
    from sklearn.model_selection import train_test_split
    from modular_semantic_segmentation_amd.experiments import split_test_data
    n = 11
    data = {'rgb': np.arange(n * 2).reshape(n, 2), 'labels': np.arange(n)}
    measure, test = split_test_data(data)
    ref_measure, ref_test = train_test_split(np.arange(n), test_size=.5, random_state=1)
    assert measure['labels'].tolist() == ref_measure.tolist() and test['labels'].tolist() == ref_test.tolist()
    assert sorted(measure['labels'].tolist() + test['labels'].tolist()) == list(range(n))
    assert np.array_equal(measure['rgb'][:, 0] // 2, measure['labels'])


def test_adapnet_weight_transforms_on_cpu():
    """adapnet.conv7s2_as_3x3 / dilated_pair_as_1x1 with numpy stand-ins for the two gather kernels reproduce
    the strided / atrous convs of adapnet.py:84-88,127 ([TF1] 'same' padding), and the variable schema matches the
    oracle's."""
    import torch
    import torch.nn.functional as F
    from modular_semantic_segmentation_amd import adapnet
    from oracle import adapnet_oracle as ao
    rng = np.random.default_rng(0)
    wt = lambda w: torch.from_numpy(w).permute(3, 2, 0, 1).contiguous()                      # noqa: E731
    nchw = lambda x: torch.from_numpy(x).permute(0, 3, 1, 2).contiguous()                    # noqa: E731
    nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()                                           # noqa: E731

    x = rng.integers(-3, 4, (1, 12, 16, 4)).astype(np.float32)
    k7 = rng.integers(-2, 3, (7, 7, 4, 5)).astype(np.float32)
    ho, wo, c = 6, 8, 4
    z = np.zeros((1, ho, wo, 9 * c), np.float32)
    xp = np.pad(x, ((0, 0), (0, 4), (0, 4), (0, 0)))
    offs = (0, 2, 1)                                                        # variants (p,s) = (0,0), (0,1), (1,0)
    for rv in range(3):
        for cv in range(3):
            g = rv * 3 + cv
            z[..., g * c:(g + 1) * c] = xp[:, offs[rv]:offs[rv] + 2 * ho:2, offs[cv]:offs[cv] + 2 * wo:2]
    got = F.conv2d(nchw(z), wt(adapnet.conv7s2_as_3x3(k7)), padding=1)
    want = F.conv2d(F.pad(nchw(x), (2, 3, 2, 3)), wt(k7), stride=2)
    assert np.array_equal(nhwc(got), nhwc(want))

    x = rng.integers(-3, 4, (1, 9, 11, 3)).astype(np.float32)
    k1 = rng.integers(-2, 3, (3, 3, 3, 2)).astype(np.float32)
    k2 = rng.integers(-2, 3, (3, 3, 3, 2)).astype(np.float32)
    for d1, d2 in ((1, 2), (2, 16)):
        cols = []
        for d in (d1, d2):
            xp = np.pad(x, ((0, 0), (d, d), (d, d), (0, 0)))
            cols += [xp[:, d + ty * d:d + ty * d + 9, d + tx * d:d + tx * d + 11] for ty in (-1, 0, 1) for tx in (-1, 0, 1)]
        z = np.concatenate(cols, axis=-1)
        got = F.conv2d(nchw(z), wt(adapnet.dilated_pair_as_1x1(k1, k2)))
        want = torch.cat([F.conv2d(nchw(x), wt(k1), padding=d1, dilation=d1),
                          F.conv2d(nchw(x), wt(k2), padding=d2, dilation=d2)], dim=1)
        assert np.array_equal(nhwc(got), nhwc(want))

    shapes = adapnet.variable_shapes('rgb', 3, 20, 14)
    assert shapes['rgb/first_deconvolution_upconv/kernel'] == (4, 4, 20, 2048)
    assert shapes['rgb/block_layer_7/stage_2_1/kernel'] == (3, 3, 128, 32) and 'rgb/block_layer_7/stage_2_1/bias' not in shapes
    assert {k: tuple(v.shape) for k, v in ao.init_adapnet_weights('rgb', 3, 20, 14).items()} == shapes
    init = adapnet.init_variables('rgb', 3, 20, 14, seed=0)
    assert np.array_equal(init['rgb/second_deconvolution_upconv/kernel'], ao.rect_bilinear_kernel(16, 14, 20))


def test_adapnet_trainer_index_maps_on_cpu():
    """adapnet_trainer.conv7s2_index_maps: the derived 3x3 kernel is a masked gather of the 7x7 one, every 7x7 tap is
    used exactly once, and mapping a filter gradient back is the adjoint of that gather."""
    from modular_semantic_segmentation_amd.adapnet import conv7s2_as_3x3
    from modular_semantic_segmentation_amd.adapnet_trainer import conv7s2_index_maps
    cin, cout = 4, 3
    src, inv = conv7s2_index_maps(cin, cout)
    rng = np.random.default_rng(0)
    w7 = rng.standard_normal((7, 7, cin, cout)).astype(np.float32)
    derived = np.where(src >= 0, w7.ravel()[np.maximum(src, 0)], 0).reshape(3, 3, 9 * cin, cout)
    assert np.array_equal(derived, conv7s2_as_3x3(w7))
    assert sorted(src[src >= 0].tolist()) == list(range(49 * cin * cout)) and np.array_equal(src[inv], np.arange(49 * cin * cout))
    dw3 = rng.standard_normal(derived.shape).astype(np.float32)
    dw7 = dw3.ravel()[inv].reshape(w7.shape)
    # <derive(w7), dw3> == <w7, back(dw3)>
    assert np.isclose((derived.astype(np.float64) * dw3).sum(), (w7.astype(np.float64) * dw7).sum())


def test_fit_writes_a_json_lines_training_log(tmp_path):
    """The reference's tf.summary scalars (base_model.py:226-251: loss, accuracy, IoU, one per additional dataset, every
    validation interval) land in output_dir/training_log.jsonl."""
    import json

    class _Trainable(base_model.BaseModel):
        def _build_graph(self):
            self.prediction, self.loss = 'label', None

        def _train_batch(self, batch):
            return 0.5

        def score(self, data, max_iterations=None):
            return {'total_accuracy': 0.75, 'mean_IoU': 0.4 if data == 'val' else 0.9}, None

    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, 12)
    net = _Trainable(desc, output_dir=str(tmp_path), device='cpu', batchsize=2)
    net.fit({'labels': np.arange(6)}, 5, output=False, validation_dataset='val', validation_interval=2,
            additional_eval_datasets={'other': 'extra'})
    rows = [json.loads(line) for line in open(os.path.join(str(tmp_path), 'training_log.jsonl'))]
    assert [r['step'] for r in rows] == [0, 2, 4] and rows[-1]['global_step'] == 5
    assert rows[0] == {'step': 0, 'global_step': 1, 'loss': 0.5, 'accuracy': 0.75, 'IoU': 0.4, 'other': 0.9}


@pytest.mark.parametrize('k,s', [(4, 2), (16, 8)])
def test_dense_deconv_phase_decomposition(k, s):
    """custom_layers.dense_deconv_as_conv3x3: a [k,k,out,in] transposed-conv kernel (k = 2*stride, 'same') as ONE 3x3
    'same' conv over the s*s output phases -- equal to the oracle's conv_transpose ([TF1] pad (k - s) // 2) after a
    depth-to-space."""
    import torch
    import torch.nn.functional as F
    from modular_semantic_segmentation_amd.custom_layers import dense_deconv_as_conv3x3
    from oracle import fcn_oracle as fo
    rng = np.random.default_rng(k)
    cin, cout = 5, 3
    W = rng.standard_normal((k, k, cout, cin)).astype(np.float32)
    x = torch.from_numpy(rng.standard_normal((2, cin, 7, 9)).astype(np.float32))
    ref = fo.deconv_same(x, W, s)
    z = F.conv2d(x, torch.from_numpy(dense_deconv_as_conv3x3(W, s)).permute(3, 2, 0, 1).contiguous(), padding=1)
    n, _, h, w = z.shape
    y = z.view(n, s, s, cout, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, cout, h * s, w * s)
    assert float((y - ref).abs().max()) < 1e-5
    with pytest.raises(NotImplementedError):
        dense_deconv_as_conv3x3(W, s + 1)


@pytest.mark.parametrize('k,s', [(4, 2), (16, 8)])
def test_dense_deconv_index_maps_are_the_kernel_map_and_its_adjoint(k, s):
    """adapnet_trainer.dense_deconv_index_maps (AdapNet trains its deconv kernels, adapnet.py:155-163): the derived 3x3
    kernel is a gather of the transposed-conv kernel, the filter gradient flows back through the inverse gather, and
    the whole chain (3x3 conv + depth-to-space) differentiates like conv_transpose2d itself."""
    import torch
    import torch.nn.functional as F
    from modular_semantic_segmentation_amd.adapnet_trainer import dense_deconv_index_maps
    from modular_semantic_segmentation_amd.custom_layers import dense_deconv_as_conv3x3
    from oracle import fcn_oracle as fo
    rng = np.random.default_rng(k + 1)
    f, cin = 3, 5
    W = rng.standard_normal((k, k, f, cin)).astype(np.float32)
    src, inv = dense_deconv_index_maps(W.shape, s)
    K = dense_deconv_as_conv3x3(W, s)
    assert np.array_equal(np.where(src >= 0, W.ravel()[np.maximum(src, 0)], 0.0).reshape(K.shape), K)
    assert np.array_equal(np.sort(inv), np.nonzero(src >= 0)[0]) and np.array_equal(src[inv], np.arange(W.size))
    # gradients: autograd through conv_transpose2d vs the phase formulation's filter gradient gathered through inv
    x = torch.from_numpy(rng.standard_normal((2, cin, 5, 6)).astype(np.float32)).requires_grad_(True)
    Wt = torch.from_numpy(W).requires_grad_(True)
    y = F.conv_transpose2d(x, Wt.permute(3, 2, 0, 1), stride=s, padding=(k - s) // 2)
    g = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
    y.backward(g)
    Kt = torch.from_numpy(K).requires_grad_(True)
    x2 = x.detach().clone().requires_grad_(True)
    z = F.conv2d(x2, Kt.permute(3, 2, 0, 1), padding=1)
    n, _, h, w = z.shape
    # space-to-depth of the upstream gradient (phase channel (py*s + px)*f + c), as xv_space_to_depth lays it out
    gz = g.view(n, f, h, s, w, s).permute(0, 3, 5, 1, 2, 4).reshape(n, s * s * f, h, w)
    z.backward(gz)
    dW = Kt.grad.numpy().ravel()[inv].reshape(W.shape)
    assert np.abs(dW - Wt.grad.numpy()).max() < 1e-4 * np.abs(Wt.grad.numpy()).max()
    assert float((x2.grad - x.grad).abs().max()) < 1e-4 * float(x.grad.abs().max())
    assert float((fo.deconv_same(x.detach(), W, s) - y.detach()).abs().max()) < 1e-5


def test_reference_named_layer_functions_host_side(golden_dir):
    """custom_layers' reference-named entry points, the parts that need no GPU: bilinear_filter_initializer is the reference's
    constant (tests/golden/bilinear_kernels.npz, generated by importing custom_layers.py:8-25) behind a verify_shape=True
    initializer; argument checking of conv2d / deconv2d happens before any launch."""
    import numpy as np
    g = np.load(os.path.join(golden_dir, 'bilinear_kernels.npz'))
    init = custom_layers.bilinear_filter_initializer([4, 4, 3, 7])
    np.testing.assert_array_equal(init([4, 4, 3, 7]), g['k4_rect'].astype(np.float32))
    np.testing.assert_array_equal(custom_layers.bilinear_filter_initializer((16, 16, 2, 5))(), g['k16_rect'].astype(np.float32))
    with pytest.raises(ValueError):
        init([4, 4, 3, 3])
    assert custom_layers._is_relu('relu') and custom_layers._is_relu(torch.relu) and not custom_layers._is_relu(None)
    with pytest.raises(NotImplementedError):
        custom_layers._is_relu('tanh')
    assert custom_layers._square([3, 3], 'k') == 3 and custom_layers._square(8, 'k') == 8
    with pytest.raises(NotImplementedError):
        custom_layers._square([3, 5], 'kernel_size')
    with pytest.raises(KeyError):
        custom_layers._var({'a/b/kernel': 1}, 'a', 'c', 'kernel')


def test_gpu_busy_is_the_union_of_kernel_intervals(tmp_path):
    """tools/gpu_busy.py (the GPU-busy fraction of the 4-image training step in the bench line): kernels of two streams
    overlap, so busy time is the UNION of the intervals over whole steps, not the sum of durations.  Synthetic trace: 4 steps
    of [0-40] + [30-60 on a second stream] + [70-90] + the marker [90-100] per 100 ns -> 90 % busy (union), sum of durations 100 %."""
    import subprocess
    import sys
    rows = ['"Kind","Agent_Id","Queue_Id","Stream_Id","Thread_Id","Dispatch_Id","Kernel_Id","Kernel_Name","Correlation_Id",'
            '"Start_Timestamp","End_Timestamp"']
    for step in range(4):
        t = 1000 + 100 * step
        for name, a, b in (('conv_a', 0, 40), ('conv_b', 30, 60), ('small', 70, 90), ('adam_kernel(float*)', 90, 100)):
            rows.append('"KERNEL_DISPATCH","Agent 2",1,0,1,1,1,"%s",1,%d,%d' % (name, t + a, t + b))
    trace = tmp_path / 'trace.csv'
    trace.write_text('\n'.join(rows) + '\n')
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'gpu_busy.py')
    out = json.loads(subprocess.run([sys.executable, tool, str(trace), '--last', '3'], capture_output=True, text=True, check=True).stdout)
    assert out['steps'] == 3 and out['kernels_per_step'] == 4.0
    assert abs(out['gpu_busy_frac'] - 0.9) < 1e-9          # window = from the end of a marker to the end of the last: 3 x 100 ns,
    #                                                         busy 3 x (60 + 20 + 10) = 270 (the marker itself counts: it is GPU work)
    assert abs(out['kernel_sum_ms_per_step'] * 1e6 - 100) < 1e-6


def test_variable_dict_caches_check_identity():
    """The functional entry points cache packed weights / engines per variables dict (key: id(dict), like a TF variable scope
    with reuse); an entry keeps its dict alive and checks identity, so a freed dict's id -- which Python hands to the next
    dict -- can never answer with the old weights."""
    a = {'x': 1}
    key = ('conv', id(a), 'm/l/kernel')
    custom_layers._cache_put(key, a, 'packed a')
    assert custom_layers._cache_get(key, a) == 'packed a'
    assert custom_layers._cache_get(key, {'x': 1}) is None          # another dict, even an equal one, under the same key
    custom_layers.clear_layer_cache()
    assert custom_layers._cache_get(key, a) is None


def test_fp8_guard_bound_from_the_model_config():
    """The accuracy guard of calibrate() (basic_fusion_model.fp8_guard_bound): on by default at 0.995, a bound of the caller's,
    off at 0 / None, and never second-guessing an explicit plan."""
    from modular_semantic_segmentation_amd.basic_fusion_model import fp8_guard_bound
    from modular_semantic_segmentation_amd.fcn import FP8_GUARD_AGREEMENT, FP8_GUARD_CANDIDATES
    assert FP8_GUARD_AGREEMENT == 0.995 and FP8_GUARD_CANDIDATES[0] == fcn.FP8_DEFAULT_START
    assert fp8_guard_bound({}) == 0.995 and fp8_guard_bound({'fp8_agreement': 0.99}) == 0.99
    assert fp8_guard_bound({'fp8_agreement': 0}) is None and fp8_guard_bound({'fp8_agreement': None}) is None
    assert fp8_guard_bound({'fp8_start': 'conv3_1'}) is None and fp8_guard_bound({'fp8_deep': True}) is None
    assert fp8_guard_bound({'fp8_start': {'rgb': 'conv2_2', 'depth': 'bf16'}}) is None
    # every candidate is a plan fp8_plan accepts
    for start in FP8_GUARD_CANDIDATES:
        convs, maps = fcn.fp8_plan(start=start)
        assert convs[0] == start and 'conv5_3' in convs


def test_result_collects_never_wait_on_their_own_pool():
    """ResultFetcher's collect tasks wait for sub-copies on the shared staging pool; they run on a pool of their
    own, so forty of them in flight (far more than the eight staging workers) all finish."""
    from modular_semantic_segmentation_amd import host_pipeline as hp
    assert hp._collect_pool() is not hp._pool()
    src = np.arange(1 << 18, dtype=np.uint8).reshape(64, -1)

    def collect():
        dst = np.empty(src.shape, np.int64)
        for f in hp._parallel_copy(dst, src, 64):
            f.result()
        return bool((dst == src).all())

    futures = [hp._collect_pool().submit(collect) for _ in range(40)]
    assert all(f.result(timeout=120) for f in futures)


def test_padded_units():
    """Decoder widths: 64 / 128 / 256 lanes (every kernel behind them, the batch-norm passes included, takes those), multiples
    of 64 beyond."""
    from modular_semantic_segmentation_amd.fcn import padded_units
    from modular_semantic_segmentation_amd.trainer import _ups8_channels_ok
    assert [padded_units(u) for u in (1, 20, 64, 65, 128, 129, 160, 192, 256, 257, 300)] == \
        [64, 64, 64, 128, 128, 256, 256, 256, 256, 320, 320]
    assert all(_ups8_channels_ok(padded_units(u)) for u in range(1, 257)) and not _ups8_channels_ok(192)


def test_adapnet_block_b_shapes_take_the_implicit_pair():
    """Every block_b of the reference's AdapNet (adapnet.py:84-88 through BLOCKS) has a shape xv_conv_dilated_pair_fwd takes --
    inference materialises no im2col operand -- and the packed [1,1,18C,F] image is block-diagonal as that kernel assumes."""
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd.adapnet import BLOCKS, dilated_pair_as_1x1
    pairs = [args for _, kind, args in BLOCKS if kind == 'b']
    assert len(pairs) == 8 and all(ops.dilated_pair_implicit_ok(f1, f2) for f1, f2, *_ in pairs)
    assert not ops.dilated_pair_implicit_ok(64, 128) and not ops.dilated_pair_implicit_ok(96, 256)
    rng = np.random.default_rng(0)
    k1, k2 = rng.standard_normal((3, 3, 8, 4)).astype(np.float32), rng.standard_normal((3, 3, 8, 4)).astype(np.float32)
    w = dilated_pair_as_1x1(k1, k2)[0, 0]
    assert w.shape == (144, 8) and not w[:72, 4:].any() and not w[72:, :4].any()
    assert np.array_equal(w[:72, :4], k1.reshape(72, 4)) and np.array_equal(w[72:, 4:], k2.reshape(72, 4))


def test_fp8_plan_and_the_oracle_policy_agree():
    """fcn.fp8_plan (which convs take e4m3 operands, which maps are stored as e4m3, by `deep`) against the
    oracle's restatement of the rule: the oracle's 'fp8' policy must quantise exactly the maps the plan names."""
    from modular_semantic_segmentation_amd.fcn import FP8_CONVS, fp8_plan, init_variables
    from oracle import fcn_oracle as fo
    for hw in ((64, 96), (384, 768), (1024, 2048)):             # the same plan on every map size (partial tiles are handled)
        convs, maps = fp8_plan(*hw)                             # round 5: conv2_1 stays bf16 and writes the first e4m3 map
        assert convs == FP8_CONVS and maps == ('conv2_1',) + FP8_CONVS
        convs, maps = fp8_plan(*hw, start='conv2_1')            # the plan of rounds 2-4
        assert convs == ('conv2_1',) + FP8_CONVS and maps == ('conv1_2', 'conv2_1') + FP8_CONVS
        convs, maps = fp8_plan(*hw, deep=True)
        assert convs == ('conv1_2', 'conv2_1') + FP8_CONVS and maps == ('conv1_1', 'conv1_2', 'conv2_1') + FP8_CONVS
        assert fp8_plan(*hw, start='conv4_1') == (FP8_CONVS[4:], FP8_CONVS[3:])
    with pytest.raises(ValueError):
        fp8_plan(start='conv1_1')
    for late in ('conv5_2', 'conv5_3'):         # would leave conv4_3 / conv5_3 in bf16 under e4m3-packed score-conv weights
        with pytest.raises(ValueError):
            fp8_plan(start=late)
    assert fp8_plan(start='conv5_1') == (FP8_CONVS[7:], FP8_CONVS[6:])
    # the oracle on a 32x48 image (partial tiles): a map is on the e4m3 grid of its scale iff the plan stores it
    wts = init_variables('rgb', 3, 64, 12, seed=4)
    x = np.random.default_rng(0).integers(0, 256, (1, 32, 48, 3)).astype(np.float32)
    names = ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2']
    allmaps = ('conv1_1', 'conv1_2', 'conv2_1') + FP8_CONVS
    plain = fo.fcn_forward(x, wts, 'rgb', 'bf16', keep=allmaps)
    scales = {n: fo.fp8_scale_exp(np.abs(plain[n]).max(), 1) for n in allmaps}
    for kw in ({}, {'start': 'conv2_1'}, {'deep': True}):
        out = fo.fcn_forward(x, wts, 'rgb', 'fp8', keep=names, fp8_scales=scales, fp8_deep=kw.get('deep', False),
                             fp8_start=kw.get('start'))
        _, maps = fp8_plan(32, 48, **kw)
        for n in names:
            on_grid = np.array_equal(out[n], fo.round_e4m3(out[n], scales[n]))
            assert on_grid == (n in maps), (kw, n)


def test_bench_launcher_parent_never_touches_the_gpu(monkeypatch, tmp_path):
    """`python bench.py --gpus N` (no launcher around it): the parent that starts torch.distributed.run must make no
    torch.cuda call -- torch.cuda.device_count() falls through to hipGetDeviceCount (which opens /dev/kfd and initialises
    the HSA runtime) whenever its amdsmi probe fails, and a process that has initialised the GPU must never be followed by an
    exec on this pool.  Every torch.cuda entry that could reach the driver is booby-trapped here; the
    GPU count comes from the KFD topology in sysfs."""
    import importlib
    import sys
    import types
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(root)
    bench = importlib.import_module('bench')
    import torch

    def boom(*a, **k):
        raise AssertionError('the launcher parent called into torch.cuda')
    for name in ('device_count', 'is_available', 'init', 'current_device', 'set_device', 'get_device_name', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, boom)
    if hasattr(torch._C, '_cuda_getDeviceCount'):
        monkeypatch.setattr(torch._C, '_cuda_getDeviceCount', boom)

    started = {}

    class FakeProc:
        stdout = iter(['{"metric": "x"}\n'])

        def wait(self):
            return 0

    def fake_popen(cmd, **kw):
        started['cmd'] = cmd
        started['env'] = kw.get('env', {})
        return FakeProc()
    monkeypatch.setattr(bench.subprocess, 'Popen', fake_popen)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '8'])
    # 8 GPUs + 2 CPU nodes in a fake topology
    nodes = tmp_path / 'nodes'
    for i in range(10):
        d = nodes / str(i)
        d.mkdir(parents=True)
        (d / 'properties').write_text('cpu_cores_count %d\nsimd_count %d\n' % (0 if i >= 2 else 64, 1024 if i >= 2 else 0))
    real_glob = importlib.import_module('glob').glob
    monkeypatch.setattr('glob.glob', lambda pat: real_glob(str(nodes / '*' / 'properties')) if 'kfd' in pat else real_glob(pat))
    assert bench.sysfs_gpu_count() == 8
    monkeypatch.setenv('HIP_VISIBLE_DEVICES', '0,1')
    assert bench.sysfs_gpu_count() == 2
    monkeypatch.delenv('HIP_VISIBLE_DEVICES')
    args = types.SimpleNamespace(gpus=8, share_device=False)
    with pytest.raises(SystemExit) as e:
        bench.launch_ranks(args)
    assert e.value.code == 0
    assert '--nproc-per-node' in started['cmd'] and started['cmd'][started['cmd'].index('--nproc-per-node') + 1] == '8'
    assert '127.0.0.1' in started['cmd'] and started['env'].get('HSA_ENABLE_IPC_MODE_LEGACY') == '0'
    # fewer GPUs than ranks: refused before anything is started
    started.clear()
    args = types.SimpleNamespace(gpus=16, share_device=False)
    with pytest.raises(SystemExit) as e:
        bench.launch_ranks(args)
    assert e.value.code == 2 and not started


def test_bench_dump_outputs_fixed_sample_under_the_size_cap(monkeypatch, tmp_path):
    """`bench.py --dump-outputs DIR`: float32 (float64 kept), whole arrays while they fit, over the cap every array cut to
    the same fixed sample, so that two runs with the same arguments write the same files."""
    import importlib
    monkeypatch.syspath_prepend(ROOT)
    bench = importlib.import_module('bench')
    labels = np.arange(4 * 8 * 16).reshape(4, 8, 16) % 12
    bench.dump_outputs(str(tmp_path / 'small'), {'labels': labels, 'loss': np.array([2.5])})
    got = np.load(tmp_path / 'small' / 'labels.npy')
    assert got.dtype == np.float32 and np.array_equal(got, labels)
    assert np.load(tmp_path / 'small' / 'loss.npy').dtype == np.float64
    monkeypatch.setattr(bench, 'DUMP_BYTES', 40000)
    big = {'params': np.random.default_rng(0).standard_normal(30000).astype(np.float32), 'labels': labels}
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), big)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['labels.npy', 'params.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 40000
    for f in files:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.size > 0 and np.array_equal(a, b)
    assert np.isin(np.load(tmp_path / 'a' / 'params.npy'), big['params']).all()


def _environment_reads():
    """{variable: [file:line, ...]} of every environment read in csrc/ and in the package; an occurrence of getenv / environ
    whose variable cannot be read off the same line (a computed name, an alias) is an error: it would hide a switch."""
    pkg = os.path.dirname(_lib.CSRC)
    found = {}

    def scan(path, token, patterns, skip=None):
        for no, line in enumerate(open(path), 1):
            if skip is not None and skip.match(line):
                continue
            uses = len(re.findall(token, line))
            names = [n for p in patterns for n in re.findall(p, line)]
            assert len(names) >= uses, '%s:%d reads the environment by a name this test cannot see: %s' % (path, no, line.strip())
            for n in names:
                found.setdefault(n, []).append('%s:%d' % (os.path.relpath(path, ROOT), no))

    for name in sorted(os.listdir(_lib.CSRC)):
        if name.endswith(('.hip', '.h')):
            scan(os.path.join(_lib.CSRC, name), r'\bgetenv\b', [r'\bgetenv\(\s*"(\w+)"\s*\)'])
    quoted = r'''['"](\w+)['"]'''
    for base, _, files in os.walk(pkg):
        for name in sorted(files):
            if name.endswith('.py'):
                scan(os.path.join(base, name), r'\benviron\b|\bgetenv\b',
                     [r'\benviron\.get\(\s*' + quoted, r'\benviron\[\s*' + quoted + r'\s*\]', r'\bgetenv\(\s*' + quoted,
                      quoted + r'\s+(?:not\s+)?in\s+(?:os\.)?environ\b'],
                     skip=re.compile(r'\s*(from\s+os\s+import|import\s+os)\b'))
    return found


def test_environment_reads_are_the_allowlisted_ones():
    """The library and the package read these environment variables and no others.  A variable left in a shell selects
    another kernel, grid or graph without a trace in any record, so a new one is added HERE in the same commit, with its
    reason:
      XV_DIRICHLET_HEAD_PK, XV_DIRICHLET_FUSE_PK, XV_GATHER_FLAT   csrc/: test_dirichlet*_pk / the gather tests pin the packed
                                                                   forms to the scalar ones and the row gathers to the flat
                                                                   ones through exactly these
      XV_FORCE_REBUILD, XV_ALLOW_STALE_LIB                         _lib.py: build and loader control (XV_LIB, which goes
                                                                   with them, is read by tools/ only)
      XVIEW_DATA_BASEPATH                                          datasets/: where the data lives
      TMPDIR                                                       datasets/: where an in-memory dataset unpacks its archive,
                                                                   as the reference's readers do; no XV_ switch
    (XV_BENCH_RAMP_S and XV_NO_POISON live in bench.py and tests/conftest.py, outside the package.)"""
    allowed = {'XV_DIRICHLET_HEAD_PK', 'XV_DIRICHLET_FUSE_PK', 'XV_GATHER_FLAT', 'XV_FORCE_REBUILD', 'XV_ALLOW_STALE_LIB',
               'XVIEW_DATA_BASEPATH', 'TMPDIR'}
    found = _environment_reads()
    assert set(found) == allowed, {k: found.get(k, 'no longer read') for k in set(found) ^ allowed}
    in_csrc = {k for k, where in found.items() if any('csrc' in w for w in where)}
    assert in_csrc == {'XV_DIRICHLET_HEAD_PK', 'XV_DIRICHLET_FUSE_PK', 'XV_GATHER_FLAT'}


def test_chooser_and_workspace_geometry_pinned(golden_dir):
    """xv_conv2d_choose_cfg and the three filter-gradient workspace queries answer what they answered before the A/B
    environment switches were folded away (tests/golden/make_chooser_golden.py recorded the table from that commit): every
    conv layer of the BASELINE.json input sizes at 1, 8 and 16 images, k = 1 and 3, flags 0..7, the four dtype pairs.  Host
    arithmetic, no launch; the one device fact in it is the CU count (256 without a device and on MI355X), recorded in the
    table -- on another count the table says nothing."""
    import sys
    sys.path.insert(0, golden_dir)
    try:
        import make_chooser_golden
    finally:
        sys.path.remove(golden_dir)
    want = json.load(open(os.path.join(golden_dir, 'chooser_geometry.json')))
    handle = _lib.lib()
    if handle.xv_conv2d_stats_rows() != want['num_cus']:
        pytest.skip('table recorded at %d CUs, this device has %d' % (want['num_cus'], handle.xv_conv2d_stats_rows()))
    got = json.loads(json.dumps(make_chooser_golden.record(handle)))
    assert sorted(got) == sorted(want)
    for table in sorted(want):
        if got[table] != want[table]:
            keys = [k for k in want[table] if got[table].get(k) != want[table][k]] if isinstance(want[table], dict) else []
            raise AssertionError('%s differs at %d entries, e.g. %s: %s != %s' % (
                table, len(keys), keys[:1], [got[table].get(k) for k in keys[:1]], [want[table][k] for k in keys[:1]]))
    assert len(want['choose_cfg']) == 252 and all(len(v) == 32 for v in want['choose_cfg'].values())
