"""The references of test_heads_fusion_edges_gpu.py without a GPU: the float32 evaluation on the CPU stays within every
counted bound, and every random-valued case leaves at most 1 % of its pixels out of the float64 label comparison -- by the
reference and the bound alone, whatever a kernel computes."""
import numpy as np
import pytest

import test_heads_fusion_edges_gpu as t

CASES = list(t.reference_cases())


@pytest.mark.parametrize('name,ref,bound,f32,labels', CASES, ids=[c[0] for c in CASES])
def test_float32_on_the_cpu_stays_within_the_counted_bound(name, ref, bound, f32, labels):
    assert f32.dtype == np.float32 and np.isfinite(ref).all() and (np.asarray(bound) >= 0).all()
    err = np.abs(f32.astype(np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / bound)
    assert ratio.max() <= 1.0, ratio.max()
    if labels:
        assert t._left_out(ref, bound) <= t.LEFT_OUT, t._left_out(ref, bound)


@pytest.mark.parametrize('kind', t.NEAR_TIES)
def test_near_tie_rows_are_what_they_say(kind):
    """The gaps the head's label forms branch on: inside and outside the 1e-5 window of the label-only forms."""
    for C in t.HEAD_C:
        if C < (3 if kind == 'tie3' else 2):
            continue
        for hi_first in (True, False):
            S, bias, z, win, run = t._near_tie_case(C, kind, hi_first)
            gap = float(np.sort(z.astype(np.float64))[-1] - np.sort(z.astype(np.float64))[-2])
            want = {'tie2': 0.0, 'tie3': 0.0, 'equal': 0.0, 'ulp': 2.0 ** -23, 'saturated': 290.0}.get(kind)
            if want is not None:
                assert gap == want
            else:
                assert abs(gap - float(kind)) < 2.0 ** -23 and (gap <= 1e-5) == (kind == '5e-6')
            if kind not in ('tie2', 'tie3', 'equal'):
                assert (win < run) == hi_first and int(np.argmax(z)) == win
            # the logits of the interior pixels of the 2x2 image are exactly z
            zz = t._exact_logits(S, bias)
            assert t._same_bits(zz[0, 4:12, 4:12], np.broadcast_to(z, (8, 8, C)))
