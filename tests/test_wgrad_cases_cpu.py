"""tests/wgrad_cases.py without a GPU: on a whole device and on its partitions every built case lands in the regime it names and
stays within the element budget -- and the six shapes of test_conv_filter_and_bias_gradient_exact_on_integers
(tests/test_backward_gpu.py) all walk ONE tile per split on 256 CUs, which is the gap tests/test_conv_wgrad_tiles_gpu.py closes."""
import pytest

import wgrad_cases as wc

CUS = [256, 128, 64, 32, 304]


def test_split_rule_on_shapes_worked_by_hand():
    # 512 -> 512 on 256 CUs: 64 blocks, 4 splits for versions 2 and 3, 12 for version 1
    assert wc.regime(256, 3, 3, 1, 16, 128, 512, 512) == (4, 2, 2, 0)           # 8 tiles: 2, 2, 2, 2
    assert wc.regime(256, 2, 3, 5, 8, 32, 512, 512) == (4, 2, 1, 1)             # 5 tiles: 2, 2, 1, 0
    assert wc.regime(256, 3, 3, 1, 24, 96, 512, 512) == (4, 3, 3, 1)            # 9 tiles: 3, 3, 3, 0
    assert wc.regime(256, 1, 3, 1, 16, 128, 512, 512) == (8, 1, 1, 0)           # 12 splits capped at the 8 tiles
    assert wc.regime(256, 3, 1, 1, 16, 128, 512, 512) == (8, 1, 1, 0)           # 1x1: the version-1 rule whatever the switch
    assert wc.regime(256, 3, 3, 1, 7, 33, 64, 64) == (2, 1, 1, 0)               # ragged 7 x 33: 1 x 2 tiles
    assert wc.regime(256, 3, 3, 1, 8, 32, 1024, 1024) == (1, 1, 1, 0)           # never fewer than one split
    # the decode across an image boundary: 2 images of 2 x 2 tiles, 13 x 40 pixels, one split of 8 tiles
    row, = wc.walk(1, 3, 3, 2, 13, 40, 1024, 1024)
    assert row == [(0, 0, 0, False), (0, 0, 1, True), (0, 1, 0, True), (0, 1, 1, True),
                   (1, 0, 0, False), (1, 0, 1, True), (1, 1, 0, True), (1, 1, 1, True)]
    assert wc.wgrad1_gi(512, 64) == 0 and wc.wgrad1_gi(128, 64) == 0 and wc.wgrad1_gi(256, 128) == 4 and wc.wgrad1_gi(128, 256) == 2


@pytest.mark.parametrize('cus', CUS)
def test_every_built_case_is_in_its_regime_and_within_budget(cus):
    cases = wc.build_cases(cus)
    assert sorted((c.name, c.kind) for c in cases) == sorted((n, k) for n in wc.REGIMES for k in wc.KINDS)
    for c in cases:
        assert wc.claims(c, cus) == [], (wc.case_id(c), c)
        assert wc.map_elems(c) <= wc.MAX_MAP_ELEMS, (wc.case_id(c), c, wc.map_elems(c))
        assert c.n * c.h * c.w <= wc.MAX_PIXELS, (wc.case_id(c), c)
        assert c.variants == wc.KINDS[c.kind][1] and c.k == wc.KINDS[c.kind][0]
    by = {(c.name, c.kind): c for c in cases}
    for kind in wc.KINDS:
        c = by['long_walk_edges', kind]
        assert c.h % wc.TH and c.w % wc.TW and c.n >= 2
        assert by['pairs_unequal', kind].cin != by['pairs_unequal', kind].cout


def test_claims_notice_a_case_built_for_another_cu_count():
    """The guard has teeth: the 256-CU cases are not all in their regimes on half the device."""
    assert any(wc.claims(c, 128) for c in wc.build_cases(256))
    assert any(wc.claims(c, 256) for c in wc.build_cases(304))


def test_budget_comes_from_the_whole_device_with_headroom():
    largest = max(wc.map_elems(c) for c in wc.build_cases(256))
    assert largest <= wc.MAX_MAP_ELEMS <= 2 * largest


@pytest.mark.parametrize('variant', [1, 2, 3])
@pytest.mark.parametrize('n,h,w,cin,cout,k', [(2, 16, 32, 64, 64, 3), (1, 24, 40, 128, 64, 3), (2, 6, 10, 64, 128, 3),
                                              (1, 20, 36, 128, 64, 1), (3, 8, 8, 512, 64, 1), (2, 16, 32, 128, 256, 3)])
def test_the_existing_exact_test_walks_one_tile_per_split(n, h, w, cin, cout, k, variant):
    splits, per, last, empty = wc.regime(256, variant, k, n, h, w, cin, cout)
    assert per == 1 and last == 1 and empty == 0 and splits == wc.tiles_of(n, h, w)[2]
