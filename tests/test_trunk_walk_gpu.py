"""One walk of the VGG16 trunk (fcn.Vgg16Walk) behind both its callers: with the same weights, re-keyed from the expert's
'<prefix>/<layer>/...' to the joint model's '<prefix>_<layer>/...' (vgg16.py:18-37), every map of fusion_fcn.VggTrunk.forward's
layer dict carries the bits of the same-named map of a bf16 fcn.FcnEngine.encoder, route bytes included -- for the three
forms of the walk (inference, keep_all, keep_all + routed: the training step) at the two smallest shapes that take different
paths:

  1 x 32 x 64, 3 channels   tiles in 16x32: conv1_1 + conv1_2 + pool1 are one launch without keep_all, and conv1_2 leaves route
                            bytes when routed (its input tiles in 32x64); pool4 is 2x4
  2 x 48 x 80, 1 channel    multiples of 16 but the width not of 32: the two-kernel first layer, partial tiles, no route kernel
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U, C = 8, 3
SHAPES = [(1, 32, 64, 3), (2, 48, 80, 1)]
FORMS = [dict(keep_all=False), dict(keep_all=True), dict(keep_all=True, routed=True)]


@pytest.fixture(scope='module')
def pairs():
    """shape -> (input, FcnEngine, VggTrunk over the same weights), built once"""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import fcn, fusion_fcn
    out = {}
    for i, shape in enumerate(SHAPES):
        cin = shape[3]
        v = fcn.init_variables('p', cin, U, C, seed=10 + i)
        rng = np.random.default_rng(20 + i)
        for name, _, _ in fcn.ENCODER:       # zero biases would leave the bias path untested
            v['p/%s/bias' % name] = rng.uniform(-0.1, 0.1, v['p/%s/bias' % name].shape).astype(np.float32)
        rekeyed = {'p_' + k[2:]: a for k, a in v.items() if k.split('/')[1].startswith('conv')}
        x = torch.from_numpy(rng.integers(0, 256, shape).astype(np.float32)).cuda()
        out[shape] = (x, fcn.FcnEngine('p', cin, U, C, v), fusion_fcn.VggTrunk('p', cin, rekeyed, 'cuda'))
    return out


@pytest.mark.parametrize('form', FORMS, ids=['inference', 'keep_all', 'routed'])
@pytest.mark.parametrize('shape', SHAPES, ids=['1x32x64x3', '2x48x80x1'])
def test_trunk_maps_equal_the_experts(pairs, shape, form):
    x, eng, trunk = pairs[shape]
    Le = eng.encoder(x, **form)
    Lt = trunk.forward(x, **form)
    torch.cuda.synchronize()
    # the same layer dict, up to what the expert's encoder adds behind the trunk
    assert set(Le) - set(Lt) == {'score_conv4', 'score_conv5', 'fused'} and set(Lt) <= set(Le)
    assert {'conv4_3', 'conv5_3', 'pool1', 'pool2', 'pool3', 'pool4'} <= set(Lt)
    tiles = shape[2] % 32 == 0
    # which path ran: the one-launch first pair writes no conv1_1; the route kernel replaces the full map by route bytes
    assert ('conv1_1' in Lt) == (form['keep_all'] or not tiles)
    routes = sorted(k for k in Lt if k.startswith('route_'))
    if form.get('routed') and tiles:
        assert 'route_conv1_2' in routes and 'conv1_2' not in Lt and 'route_conv4_3' not in routes
    else:
        assert not routes
    assert len(Lt) == (17 if form['keep_all'] else 13 if tiles else 14)      # 13 convs + 4 pools; inference keeps 9 + 4 (+ conv1_1)
    for name, got in Lt.items():
        want = Le[name]
        if name.startswith('route_'):
            assert got.dtype == torch.uint8 and torch.equal(got, want), name
        else:
            assert (got.n, got.h, got.w, got.c, got.dtype) == (want.n, want.h, want.w, want.c, 'bf16'), name
            assert torch.equal(got.interior().view(torch.int16), want.interior().view(torch.int16)), name
    assert float(Lt['conv5_3'].interior().float().abs().max()) > 0          # not a comparison of zero maps
