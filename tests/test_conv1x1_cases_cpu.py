"""tests/conv1x1_cases.py without a GPU: on a whole device and on its partitions every built case lands in the form and has the
properties its row names; the integer operands keep every sum exact; the float64 reference is the convolution it claims to
be and its mask select tells +-0 and the smallest normal apart; the tolerance of the real-valued test holds for a float32
evaluation that involves no kernel; and the library's chooser query names the flat-GEMM configurations for the cases."""
import numpy as np
import pytest

import conv1x1_cases as cc

CUS = [256, 64, 128, 304, 80]

# worked by hand for 256 CUs: (form, n, h, w, K, C) -> Mp, workgroups, remap, whole last tile
BY_HAND = [
    ('g128', 1, 6, 10, 256, 128, 96, 1, False, False),
    ('g128', 3, 7, 5, 512, 384, 189, 6, False, False),
    ('g128', 2, 12, 20, 256, 1024, 616, 40, True, False),
    ('wide', 3, 25, 50, 512, 512, 4212, 68, False, False),
    ('wide', 4, 30, 33, 256, 1024, 4480, 144, True, False),
    ('wide', 4, 30, 30, 256, 512, 4096, 64, True, True),
    ('n64', 1, 5, 7, 128, 64, 63, 1, False, False),
    ('n64', 3, 7, 5, 512, 64, 189, 3, False, False),
    ('n64', 2, 30, 30, 256, 64, 2048, 32, False, True),
]


@pytest.mark.parametrize('form,n,h,w,k,c,mp,nblk,remap,whole', BY_HAND)
def test_geometry_on_shapes_worked_by_hand(form, n, h, w, k, c, mp, nblk, remap, whole):
    g = cc.geometry(256, n, h, w, k, c)
    assert (g.form, g.mp, g.nblk, g.remap, g.whole) == (form, mp, nblk, remap, whole)
    assert g.cfg == (23 if form == 'n64' else 18) and g.ksteps == k // 64


def test_form_thresholds():
    # 4 ceil(Mp / 256) (C / 128) >= cus: 64 wide workgroups are a quarter of a round of 256 CUs, 63 are not
    assert cc.geometry(256, 4, 30, 30, 256, 512).form == 'wide' and cc.geometry(257, 4, 30, 30, 256, 512).form == 'g128'
    assert cc.geometry(252, 1, 14, 14, 256, 128 * 63).form == 'wide' and cc.geometry(253, 1, 14, 14, 256, 128 * 63).form == 'g128'
    # channel rules: 18 from 256 reduction channels onto whole 128s, 23 from 128 onto exactly 64
    assert cc.geometry(256, 1, 8, 8, 192, 128).form == 'gen1' and cc.geometry(256, 1, 8, 8, 320, 128).form == 'g128'
    assert cc.geometry(256, 1, 8, 8, 256, 192).form == 'gen1' and cc.geometry(256, 1, 8, 8, 64, 64).form == 'gen1'
    assert cc.geometry(256, 1, 8, 8, 128, 64).form == 'n64'
    # the shapes of the two direct tests there were (test_adapnet_gpu.py, test_backward_gpu.py) stay on generation 1
    assert cc.geometry(256, 2, 10, 14, 128, 256).cfg == 1 and cc.geometry(256, 1, 20, 36, 64, 128).form == 'gen1'
    assert cc.gen1_cfg(8, 40, 64, 64) == 15 and cc.gen1_cfg(10, 14, 64, 128) == 14 and cc.gen1_cfg(17, 14, 128, 128) == 1


@pytest.mark.parametrize('cus', CUS + [32])
def test_every_row_is_built_and_has_its_properties(cus):
    cases = cc.build_cases(cus)
    assert [(c.form, c.prop) for c in cases] == [r for r in cc.ROWS if r not in cc.unreachable(cus)]
    assert cc.unreachable(cus) == ((('g128', 'remap_tail'),) if cus == 32 else ())
    for c in cases:
        assert cc.claims(c, cus) == [], (cc.case_id(c), c)
        g = cc.geometry(cus, c.n, c.h, c.w, c.k, c.c)
        assert g.form == c.form and g.cfg == {'g128': 18, 'wide': 18, 'n64': 23}.get(c.form, g.cfg)
        # no case larger than the largest of the hand-worked table: 4480 rows x 1024 channels, 1.2 G products
        assert cc.map_elems(c) <= 4480 * 1024 and g.mp * c.k * c.c <= 1.25e9, (cc.case_id(c), c)
        assert cc.max_abs_sum(c) < 2 ** 24
    assert {c.form for c in cases} == set(cc.FORMS)


def test_unreachable_row_is_unreachable():
    """On 32 CUs no shape of the grid is in g128 with the remap: the builder leaves the row out instead of bending it."""
    for k in (256,):
        for c in (256, 512, 1024):
            for n in (1, 2, 3):
                for h in range(4, 34, 3):
                    for w in range(4, 53, 3):
                        g = cc.geometry(32, n, h, w, k, c)
                        assert not (g.form == 'g128' and g.remap and g.nblk >= 16)


def test_claims_notice_a_case_built_for_another_cu_count():
    """The guard has teeth: the wide cases of a partition are not wide on the whole device, and the other way round."""
    assert any(cc.claims(c, 256) for c in cc.build_cases(64))
    assert any(cc.claims(c, 304) for c in cc.build_cases(256))
    wide = [c for c in cc.build_cases(64) if c.form == 'wide']
    assert wide and all(cc.claims(c, 256) for c in wide)


def test_integer_operands_keep_every_sum_exact():
    for cus in CUS:
        for c in cc.build_cases(cus):
            assert cc.max_abs_sum(c) < 2 ** 24
    c = cc.build_cases(256)[1]
    o = cc.draw_integers(c, 5)
    for a, top in ((o.x, cc.X_MAX), (o.w, cc.W_MAX), (o.b, cc.B_MAX), (o.addend, cc.R_MAX)):
        assert a.dtype == np.float32 and np.array_equal(a, np.round(a)) and a.min() == -top and a.max() == top
    assert float(cc.magnitude(o.x, o.w, o.b, o.addend).max()) <= cc.max_abs_sum(c)
    assert cc.draw_integers(c, 5, addend_max=3).addend.max() == 3
    assert set(np.unique(o.mask[0, 1:])) <= set(cc.MASK_VALUES)
    assert np.array_equal(o.mask[0, 0, 0, :6], np.float32(cc.SPECIAL_MASK)) and np.array_equal(o.mask[-1, -1, -1, -6:], np.float32(cc.SPECIAL_MASK))
    assert np.signbit(o.mask[0, 0, 0, 1]) and not np.signbit(o.mask[0, 0, 0, 0])


def test_reference_is_the_convolution():
    import torch
    import torch.nn.functional as F
    c = cc.Case('n64', 'one_partial', 2, 5, 7, 128, 64)
    o = cc.draw_integers(c, 7)
    conv = F.conv2d(torch.from_numpy(o.x).double().permute(0, 3, 1, 2), torch.from_numpy(o.w).double().T[:, :, None, None],
                    torch.from_numpy(o.b).double()).permute(0, 2, 3, 1)
    assert np.array_equal(cc.reference(o.x, o.w, o.b, rounded=False), conv.numpy())
    want = torch.relu(conv) + torch.from_numpy(o.addend).double()
    want = torch.where(torch.from_numpy(o.mask) > 0, want, torch.zeros_like(want))
    got = cc.reference(o.x, o.w, o.b, relu=True, addend=o.addend, mask=o.mask)
    assert got.dtype == np.float32 and np.array_equal(got, want.bfloat16().float().numpy())
    # the order is visible: the activation BEFORE the addend, the mask last
    v = conv.numpy()
    assert np.array_equal(cc.reference(o.x, o.w, o.b, relu=True, addend=o.addend, rounded=False), np.maximum(v, 0) + o.addend)
    assert (np.maximum(v, 0) + o.addend != np.maximum(v + o.addend, 0)).any()
    # one rounding, to nearest even, of the exact value: 257 -> 256 and 259 -> 260 (ties), 1027 -> 1024, 1029 -> 1032
    x = np.float32([[257, 0], [259, 0], [1027, 0], [1029, 0], [-259, 0]])
    assert cc.reference(x, np.float32([[1], [0]])).ravel().tolist() == [256, 260, 1024, 1032, -260]


def test_mask_select_on_the_special_values():
    v = np.float32([[5, -7, 11, -13, 17, -19]])
    got = cc.reference(np.eye(6, dtype=np.float32), np.diag(v[0]), mask=np.float32([cc.SPECIAL_MASK] * 6), rounded=False)
    assert np.array_equal(np.diag(got), np.where(cc.SPECIAL_KEEPS, v[0], 0)) and not np.signbit(np.diag(got)[1])
    ones = cc.reference(np.ones((1, 1), np.float32), np.full((1, 6), 7, np.float32), mask=np.float32([cc.SPECIAL_MASK]))
    assert ones.tolist() == [[0, 0, 7, 0, 7, 0]]
    # the smallest positive normal survives the storage format: bf16 keeps float32's exponent range
    from oracle.fcn_oracle import round_bf16
    assert float(round_bf16(np.float32([cc.TINY]))[0]) == cc.TINY > 0


REAL_ROWS = [('g128', 'remap_tail'), ('wide', 'noremap_tail'), ('n64', 'tiles_tail'), ('gen1', 'k128')]


@pytest.mark.parametrize('row', REAL_ROWS, ids=['%s-%s' % r for r in REAL_ROWS])
def test_tolerance_holds_for_a_float32_evaluation(row):
    """The bound of the real-valued GPU test, on the same operands, for numpy's float32 matrix product (its own summation
    order) + float32 epilogue + one bf16 rounding: satisfiable without the kernel, and not by a wide margin in the first term."""
    from oracle.fcn_oracle import round_bf16
    c = {(c.form, c.prop): c for c in cc.build_cases(256)}[row]
    o = cc.draw_reals(c, 40 + REAL_ROWS.index(row))
    for relu, mask in ((True, None), (False, o.mask)):
        ref = cc.reference(o.x, o.w, o.b, relu=relu, addend=o.addend, mask=mask, rounded=False)
        tol = cc.tolerance(ref, cc.magnitude(o.x, o.w, o.b, o.addend), c.k)
        v = (o.x.reshape(-1, c.k) @ o.w).reshape(ref.shape) + o.b
        assert v.dtype == np.float32
        v = (np.maximum(v, 0) if relu else v) + o.addend
        v = v if mask is None else np.where(mask > 0, v, np.float32(0))
        ratio = np.abs(round_bf16(v).astype(np.float64) - ref) / np.maximum(tol, 1e-300)
        print('%s-%s relu %d mask %d: largest error / bound %.3f' % (row + (relu, mask is not None, ratio.max())))
        assert ratio.max() <= 1.0
        assert ratio.max() > 0.25          # bf16's half ulp is 2^-9 .. 2^-8 of the value: the first term is no loose one
        # ... and a relu moved behind the addend is far outside it
        if relu:
            wrong = np.maximum(cc.reference(o.x, o.w, o.b, addend=o.addend, rounded=False), 0)
            assert (np.abs(wrong - ref) > tol).mean() > 0.1


def test_chooser_query_names_the_flat_gemm_configurations():
    """xv_conv2d_choose_cfg answers what the dispatch resolves to for a 1x1 conv with a full-resolution output: 18 and 23 where
    pick_cfg takes them (host arithmetic, no launch; the CU count is the library's own, 256 without a device)."""
    from modular_semantic_segmentation_amd import _lib
    handle = _lib.lib()
    cus = handle.xv_conv2d_stats_rows()
    bf16, fp8 = _lib.CONSTANTS['XV_BF16'], _lib.CONSTANTS['XV_FP8']
    for c in cc.build_cases(cus):
        want = cc.geometry(cus, c.n, c.h, c.w, c.k, c.c).cfg
        for flags in (0, 2, 4, 6):
            assert handle.xv_conv2d_choose_cfg(c.n, c.h, c.w, c.k, c.c, 1, bf16, bf16, flags) == want, (cc.case_id(c), flags)
        # a pooled output does not exist for k = 1; e4m3 maps stay on the first generation
        assert handle.xv_conv2d_choose_cfg(c.n, c.h, c.w, c.k, c.c, 1, bf16, bf16, 1) == _lib.CONSTANTS['XV_ESHAPE']
        assert handle.xv_conv2d_choose_cfg(c.n, c.h, c.w, c.k, c.c, 1, bf16, fp8, 0) in (14, 15)
    # the 3x3 answers do not move with the output sentinel
    assert handle.xv_conv2d_choose_cfg(1, 48, 96, 512, 512, 3, bf16, bf16, 0) in (26, 27)
