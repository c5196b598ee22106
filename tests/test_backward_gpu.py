"""Parity of the backward kernels and of a full training step against PyTorch-CPU autograd over the
oracle's restatement of the training graph (simple_fcn.py:200-214, utils.py:43-53)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import fcn_oracle as fo
from oracle import fusion_oracle as fu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from modular_semantic_segmentation_amd import ops as _ops
    return _ops


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


@pytest.fixture
def default_wgrad_variant_afterwards(ops):
    """xv_set_wgrad_variant is process-wide: whatever a test that sets it does -- a failed assertion included -- the tests
    after it run the default kernel again."""
    yield
    from modular_semantic_segmentation_amd import _lib
    _lib.lib().xv_set_wgrad_variant(0)


@pytest.mark.parametrize('n,h,w,cin,cout,k', [(2, 16, 32, 64, 64, 3), (1, 24, 40, 128, 64, 3), (2, 6, 10, 64, 128, 3),
                                              (1, 20, 36, 128, 64, 1), (3, 8, 8, 512, 64, 1), (2, 16, 32, 128, 256, 3)])
@pytest.mark.parametrize('variant', [1, 2, 3])
def test_conv_filter_and_bias_gradient_exact_on_integers(ops, default_wgrad_variant_afterwards, n, h, w, cin, cout, k, variant):
    from modular_semantic_segmentation_amd import _lib
    assert _lib.lib().xv_set_wgrad_variant(variant) == 0
    rng = np.random.default_rng(cin + cout + h)
    x = rng.integers(-2, 3, (n, h, w, cin)).astype(np.float32)
    dy = rng.integers(-1, 2, (n, h, w, cout)).astype(np.float32)
    dw = torch.zeros((k, k, cin, cout), device='cuda')
    db = torch.zeros(cout, device='cuda')
    ops.conv2d_bwd_filter(ops.Act.from_dense(_dev(x)), ops.Act.from_dense(_dev(dy)), dw, db, k)
    torch.cuda.synchronize()
    wt = torch.zeros((cout, cin, k, k), requires_grad=True)
    b = torch.zeros(cout, requires_grad=True)
    F.conv2d(_nchw(x), wt, b, padding=(k - 1) // 2).backward(_nchw(dy))
    ref = wt.grad.permute(2, 3, 1, 0).numpy()              # -> HWIO
    assert np.array_equal(dw.cpu().numpy(), ref)
    assert np.array_equal(db.cpu().numpy(), b.grad.numpy())
    # slab (workspace) reduction: same sums, accumulated INTO dw, identical from run to run
    xa, dya = ops.Act.from_dense(_dev(x)), ops.Act.from_dense(_dev(dy))
    ws = torch.empty(ops.conv2d_bwd_filter_workspace_bytes(xa, cout, k) // 4, device='cuda')
    dw2 = torch.ones((k, k, cin, cout), device='cuda')
    ops.conv2d_bwd_filter(xa, dya, dw2, None, k, workspace=ws)
    torch.cuda.synchronize()
    _lib.lib().xv_set_wgrad_variant(0)          # back to the default
    assert np.array_equal(dw2.cpu().numpy(), ref + 1)


@pytest.mark.parametrize('n,h,w,cin,cout', [(2, 12, 20, 256, 128), (1, 24, 48, 512, 256), (3, 5, 7, 256, 384), (8, 24, 48, 1024, 128),
                                            (1, 6, 6, 2304, 128), (1, 1, 1, 256, 128), (2, 12, 20, 128, 256), (3, 9, 7, 128, 512)])
def test_1x1_filter_gradient_as_flat_gemm_exact_on_integers(ops, n, h, w, cin, cout):
    """conv_wgrad_1x1_gemm_kernel (1x1 convs with cin % 256 == 0, cout % 128 == 0 -- or 128 / 256 -- and a workspace: AdapNet's block stages and
    the 1x1 conv over its im2col operand): the reduction runs over all padded pixels in 64-row steps, split into slabs --
    exact on integers with and without the bias gradient, accumulated INTO dw, the same bits from run to run."""
    rng = np.random.default_rng(cin + cout + h)
    x = rng.integers(-2, 3, (n, h, w, cin)).astype(np.float32)
    dy = rng.integers(-1, 2, (n, h, w, cout)).astype(np.float32)
    wt = torch.zeros((cout, cin, 1, 1), requires_grad=True)
    b = torch.zeros(cout, requires_grad=True)
    F.conv2d(_nchw(x), wt, b).backward(_nchw(dy))
    ref = wt.grad.permute(2, 3, 1, 0).numpy()
    xa, dya = ops.Act.from_dense(_dev(x)), ops.Act.from_dense(_dev(dy))
    ws = torch.empty(ops.conv2d_bwd_filter_workspace_bytes(xa, cout, 1) // 4, device='cuda').fill_(float('nan'))
    dw = torch.ones((1, 1, cin, cout), device='cuda')
    db = torch.full((cout,), 2.0, device='cuda')
    ops.conv2d_bwd_filter(xa, dya, dw, db, 1, workspace=ws)
    torch.cuda.synchronize()
    assert np.array_equal(dw.cpu().numpy(), ref + 1) and np.array_equal(db.cpu().numpy(), b.grad.numpy() + 2)
    dw2 = torch.zeros((1, 1, cin, cout), device='cuda')
    ops.conv2d_bwd_filter(xa, dya, dw2, None, 1, workspace=ws)
    assert np.array_equal(dw2.cpu().numpy(), ref)
    # floats: bitwise reproducible, and the float32 sum to rounding
    xf = ops.Act.from_dense(_dev(rng.standard_normal((n, h, w, cin)).astype(np.float32)))
    df = ops.Act.from_dense(_dev(rng.standard_normal((n, h, w, cout)).astype(np.float32)))
    outs = []
    for _ in range(2):
        d = torch.zeros((1, 1, cin, cout), device='cuda')
        ops.conv2d_bwd_filter(xf, df, d, None, 1, workspace=ws)
        outs.append(d)
    assert torch.equal(outs[0], outs[1])
    xi, di = xf.interior().double(), df.interior().double()
    want = torch.einsum('nhwi,nhwo->io', xi, di)
    bound = 1e-5 * float(torch.einsum('nhwi,nhwo->io', xi.abs(), di.abs()).max())      # fp32 sums of exact bf16 products
    assert float((outs[0][0, 0].double() - want).abs().max()) <= bound


@pytest.mark.parametrize('k,h,w', [(3, 24, 40), (1, 24, 40), (3, 32, 64), (3, 40, 72)])
def test_conv_data_gradient_with_relu_mask_and_addend(ops, k, h, w):
    """24x40: generation-1 kernel; 32x64: whole tiles of the all-DMA generation-2 kernel with its split-phase
    epilogue; 40x72: its partial tiles (clamped offsets, predicated addend / mask loads and stores)."""
    rng = np.random.default_rng(k + h)
    n, cin, cout = 2, 128, 64
    wt = rng.integers(-1, 2, (k, k, cin, cout)).astype(np.float32)
    dy = rng.integers(-2, 3, (n, h, w, cout)).astype(np.float32)
    ref_act = rng.integers(-1, 3, (n, h, w, cin)).astype(np.float32)     # forward output of the layer below
    add = rng.integers(-3, 4, (n, h, w, cin)).astype(np.float32)
    wd = ops.pack_conv_weights_dgrad(_dev(wt))
    dx = ops.Act(n, h, w, cin)
    ops.conv2d_bwd_data(ops.Act.from_dense(_dev(dy)), wd, torch.zeros(cin, device='cuda'), dx, k,
                        relu_ref=ops.Act.from_dense(_dev(ref_act)), addend=ops.Act.from_dense(_dev(add)))
    torch.cuda.synchronize()
    xin = torch.zeros((n, cin, h, w), requires_grad=True)
    F.conv2d(xin, torch.from_numpy(wt).permute(3, 2, 0, 1), padding=(k - 1) // 2).backward(_nchw(dy))
    ref = fo.round_bf16((_nhwc(xin.grad) + add) * (ref_act > 0))
    assert np.array_equal(dx.interior().float().cpu().numpy(), ref)


def test_maxpool_relu_backward_with_ties(ops):
    rng = np.random.default_rng(1)
    n, h, w, c = 2, 12, 20, 64
    y = rng.integers(0, 3, (n, h, w, c)).astype(np.float32)          # many ties, many zeros
    dp = rng.integers(-4, 5, (n, h // 2, w // 2, c)).astype(np.float32)
    dy = ops.Act(n, h, w, c)
    ops.maxpool2x2_bwd(ops.Act.from_dense(_dev(y)), ops.Act.from_dense(_dev(dp)), dy)
    torch.cuda.synchronize()
    yt = _nchw(y).requires_grad_(True)
    F.max_pool2d(yt, 2, 2).backward(_nchw(dp))
    ref = _nhwc(yt.grad) * (y > 0)
    assert np.array_equal(dy.interior().float().cpu().numpy(), ref)


@pytest.mark.parametrize('n,h,w,cin,cout,c2', [(2, 32, 64, 64, 64, 128), (1, 64, 64, 128, 128, 64), (1, 32, 128, 64, 256, 64)])
def test_routed_pool_forward_and_data_gradient(ops, n, h, w, cin, cout, c2):
    """The routed pool of the training step (xv_conv2d_fwd_route / xv_conv2d_bwd_data_route): pooled map and route bytes with no
    full map, the data gradient of the layer behind the pool stored through the routes -- the same bits as the full map +
    xv_conv2d_bwd_data + xv_maxpool2x2_bwd (MaxPoolGrad's first maximum, ReluGrad's y > 0), on sparse integers: many ties,
    many windows without a positive value."""
    rng = np.random.default_rng(n + h + cout)
    x = (rng.integers(-2, 3, (n, h, w, cin)) * (rng.random((n, h, w, cin)) < 0.05)).astype(np.float32)
    wt = rng.integers(-1, 2, (3, 3, cin, cout)).astype(np.float32)
    b = _dev(rng.integers(-1, 2, cout).astype(np.float32))
    wp = ops.pack_conv_weights(_dev(wt))
    xa = ops.Act.from_dense(_dev(x))
    y, q = ops.conv2d_fwd(xa, wp, b, 3, relu=True, y=ops.Act(n, h, w, cout), pooled=ops.Act(n, h // 2, w // 2, cout))
    q2 = ops.Act(n, h // 2, w // 2, cout)
    route = torch.full((n * (h // 2) * (w // 2) * cout,), 77, dtype=torch.uint8, device='cuda')
    assert ops.conv2d_fwd_route(xa, wp, b, q2, route)
    torch.cuda.synchronize()
    assert torch.equal(q.t, q2.t)
    yv = y.interior().float().cpu().numpy()
    win = yv.reshape(n, h // 2, 2, w // 2, 2, cout).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, cout, 4)
    code = np.where(win.max(-1) > 0, 0x80 >> win.argmax(-1), 0)          # (numpy's argmax: the first maximum)
    got = route.view(n, h // 2, w // 2, cout).cpu().numpy()
    assert np.array_equal(got, code)
    assert 0.02 < (code == 0).mean() < 0.98 and len(np.unique(code)) == 5
    # the layer behind the pool: gradient g of its output, data gradient onto the pooled map, routed onto the full map
    w2 = rng.integers(-1, 2, (3, 3, cout, c2)).astype(np.float32)
    g = ops.Act.from_dense(_dev(rng.integers(-2, 3, (n, h // 2, w // 2, c2)).astype(np.float32)))
    wd = ops.pack_conv_weights_dgrad(_dev(w2))
    zero = torch.zeros(cout, device='cuda')
    dpool = ops.conv2d_bwd_data(g, wd, zero, ops.Act(n, h // 2, w // 2, cout), 3)
    ref = ops.maxpool2x2_bwd(y, dpool, ops.Act(n, h, w, cout))
    dx = ops.Act(n, h, w, cout)
    dx.interior().fill_(3.0)                                              # every interior value is written
    ops.conv2d_bwd_data_route(g, wd, zero, route, dx)
    torch.cuda.synchronize()
    assert torch.equal(dx.t, ref.t)
    assert dx.interior().float().abs().sum().item() > 0


def test_routed_pool_shapes_it_does_not_take(ops):
    """Maps whose pooled size does not tile in 16x32 pixels: nothing launched, the caller keeps the full map."""
    xa = ops.Act(1, 48, 96, 64)
    wp = ops.pack_conv_weights(torch.zeros(3, 3, 64, 64, device='cuda'))
    route = torch.zeros(24 * 48 * 64, dtype=torch.uint8, device='cuda')
    assert not ops.conv2d_fwd_route(xa, wp, torch.zeros(64, device='cuda'), ops.Act(1, 24, 48, 64), route)


def test_training_step_same_bits_with_and_without_routed_pool(ops, tmp_path, monkeypatch):
    """Two Adam steps of an expert at 64x128 (pool1 and pool2 take the routed form, pool3 / pool4 do not): loss, gradients and
    parameters bit-identical to the path through the full maps and xv_maxpool2x2_bwd."""
    from modular_semantic_segmentation_amd import get_model
    C, U, H, W = 12, 64, 64, 128
    rng = np.random.default_rng(5)
    data = {'rgb': rng.integers(0, 256, (2, H, W, 3)).astype(np.float32),
            'labels': rng.integers(-1, C, (2, H, W)).astype(np.int32)}
    w = fo.init_fcn_weights('rgb', 3, U, C, seed=2, bias_scale=0.02)
    w['rgb/conv1_1/kernel'] *= 0.02
    path = str(tmp_path / 'w.npz')
    np.savez(path, **w)
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, C)
    results = []
    for routed in (True, False):
        monkeypatch.setattr(ops, 'ROUTED_POOL', routed)
        net = get_model('fcn')('rgb', desc, 'rgb', output_dir=str(tmp_path), num_units=U, batch_normalization=False,
                               batchsize=2, learning_rate=1e-3, trainer='adam')
        net.import_weights(path, warnings=False)
        tr = net._ensure_trainer()
        losses = [tr.step(_dev(data['rgb']), _dev(data['labels'])).item() for _ in range(2)]
        torch.cuda.synchronize()
        L = tr.e.encoder(_dev(data['rgb']), keep_all=True, routed=True)
        assert ('route_conv1_2' in L) == routed and ('route_conv2_2' in L) == routed and 'route_conv3_3' not in L
        assert ('conv1_2' in L) != routed
        results.append((losses, tr.grad.clone(), tr.param.clone()))
    assert results[0][0] == results[1][0]
    assert torch.equal(results[0][1], results[1][1])
    assert torch.equal(results[0][2], results[1][2])


def test_relu_backward(ops):
    rng = np.random.default_rng(2)
    g = fo.round_bf16(rng.standard_normal((1, 5, 7, 64)).astype(np.float32))
    ref_act = rng.integers(-1, 2, (1, 5, 7, 64)).astype(np.float32)
    out = ops.Act(1, 5, 7, 64)
    ops.relu_bwd(ops.Act.from_dense(_dev(g)), ops.Act.from_dense(_dev(ref_act)), out)
    torch.cuda.synchronize()
    assert np.array_equal(out.interior().float().cpu().numpy(), g * (ref_act > 0))


def test_upsample2x_backward(ops):
    rng = np.random.default_rng(3)
    n, h, w, c = 2, 5, 7, 64
    s5 = fo.round_bf16(np.maximum(rng.standard_normal((n, h, w, c)), 0).astype(np.float32))
    df = fo.round_bf16(rng.standard_normal((n, 2 * h, 2 * w, c)).astype(np.float32))
    ds5 = ops.Act(n, h, w, c)
    ops.upsample2x_bwd(ops.Act.from_dense(_dev(df)), ops.Act.from_dense(_dev(s5)), ds5)
    torch.cuda.synchronize()
    st = _nchw(s5).requires_grad_(True)
    wk = torch.from_numpy(fo.bilinear_kernel(4, c)).permute(3, 2, 0, 1).contiguous()
    F.relu(F.conv_transpose2d(st, wk, stride=2, padding=1)).backward(_nchw(df))
    ref = _nhwc(st.grad) * (s5 > 0)
    got = ds5.interior().float().cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=2 ** -7, atol=1e-6)


@pytest.mark.parametrize('C', [12, 5])
def test_head_backward_loss_and_gradients(ops, C):
    rng = np.random.default_rng(C)
    n, h, w, U = 2, 3, 5, 64
    f = fo.round_bf16(np.abs(rng.standard_normal((n, h, w, U))).astype(np.float32))
    f[:, :, :, 7] = 0                                    # a dead channel: relu'(0) = 0 in the reference
    f[0, 1, 2, :] = 0
    ws = (rng.standard_normal((U, C)) * 0.3).astype(np.float32)
    bs = rng.standard_normal(C).astype(np.float32)
    lab = rng.integers(-1, C, (n, 8 * h, 8 * w)).astype(np.int32)
    count = torch.zeros(1, dtype=torch.int64, device='cuda')
    ops.count_valid_labels(_dev(lab), C, count)
    loss = torch.zeros(1, dtype=torch.float64, device='cuda')
    dws = torch.zeros((U, C), device='cuda')
    dbs = torch.zeros(C, device='cuda')
    df = ops.Act(n, h, w, U)
    ops.decoder_head_bwd(ops.Act.from_dense(_dev(f)), _dev(ws), _dev(bs), _dev(lab), count, C, loss, dws, dbs, df)
    torch.cuda.synchronize()
    assert count.item() == (lab >= 0).sum()
    ft = _nchw(f).requires_grad_(True)
    wk = torch.from_numpy(fo.bilinear_kernel(16, U)).permute(3, 2, 0, 1).contiguous()
    wst = torch.from_numpy(ws).requires_grad_(True)
    bst = torch.from_numpy(bs).requires_grad_(True)
    score = F.relu(F.conv_transpose2d(ft, wk, stride=8, padding=4)).permute(0, 2, 3, 1) @ wst + bst
    logp = F.log_softmax(score, -1)
    labt = torch.from_numpy(lab.astype(np.int64))
    valid = labt >= 0
    onehot = F.one_hot(labt.clamp(0), C).float() * valid[..., None]
    ref_loss = -(onehot * logp).sum() / (1e-20 + onehot.sum())
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-5 * max(1.0, abs(ref_loss.item()))
    np.testing.assert_allclose(dws.cpu().numpy(), wst.grad.numpy(), rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(dbs.cpu().numpy(), bst.grad.numpy(), rtol=1e-3, atol=1e-7)
    # d loss / d fused: equal to autograd wherever fused > 0; where fused == 0 the commuted form passes a
    # gradient that the relu masks of score_conv4 / upscore_conv5 (fused == 0 => both are 0) remove next
    ref_df = _nhwc(ft.grad)
    got_df = df.interior().float().cpu().numpy()
    pos = f > 0
    scale = np.abs(ref_df).max()
    np.testing.assert_allclose(got_df[pos], ref_df[pos], rtol=2 ** -7, atol=2e-3 * scale)


@pytest.mark.parametrize('shape', [(2, 12, 20), (1, 9, 22), (3, 33, 64), (5, 40, 132), (1, 3, 12), (1, 5, 28), (2, 8, 32), (3, 16, 64),
                                   (2, 24, 96)])
@pytest.mark.parametrize('cin,data', [(1, 'u8'), (3, 'u8'), (1, 'u16'), (3, 'float'), (4, 'float')])
def test_first_layer_filter_gradient(ops, cin, shape, data):
    """Maps that tile in 8x32 pixels: the bf16-split kernel (exact three-way split of X; 8-bit data skip the two lower terms,
    16-bit data the last, floats take all three); else W % 4 == 0: the fp32-MFMA kernel (the two small shapes end inside a
    wave's batch of four quads); other widths: the packed-FMA kernel."""
    rng = np.random.default_rng(cin)
    n, h, w = shape
    if data == 'u8':
        x = rng.integers(0, 256, (n, h, w, cin)).astype(np.float32)
    elif data == 'u16':
        x = rng.integers(0, 65536, (n, h, w, cin)).astype(np.float32)
    else:
        x = (rng.standard_normal((n, h, w, cin)) * 100).astype(np.float32)
    dy = fo.round_bf16(rng.standard_normal((n, h, w, 64)).astype(np.float32))
    dw = torch.zeros((3, 3, cin, 64), device='cuda')
    db = torch.zeros(64, device='cuda')
    dya = ops.Act.from_dense(_dev(dy))
    ops.conv2d_first_bwd_filter(_dev(x), dya, dw, db)
    db2 = torch.zeros(64, device='cuda')
    ops.bias_grad(dya, db2)
    torch.cuda.synchronize()
    grow = max(1.0, n * h * w / 480.0) ** 0.5          # fp32 sums over more pixels, in different orders
    np.testing.assert_allclose(db2.cpu().numpy(), db.cpu().numpy(), rtol=1e-5, atol=1e-5 * grow)
    wt = torch.zeros((64, cin, 3, 3), requires_grad=True)
    b = torch.zeros(64, requires_grad=True)
    F.conv2d(_nchw(x), wt, b, padding=1).backward(_nchw(dy))
    ref = wt.grad.permute(2, 3, 1, 0).numpy()
    np.testing.assert_allclose(dw.cpu().numpy(), ref, rtol=1e-4, atol=max(1e-2 * grow, 2e-5 * np.abs(ref).max()))       # (fp32 sums of terms up to 65535 x |dy|)
    np.testing.assert_allclose(db.cpu().numpy(), b.grad.numpy(), rtol=1e-4, atol=1e-4 * grow)
    # with a workspace: the same sums in a fixed order -- bit for bit the same on every run, and within fp32 rounding of the above
    ws = torch.empty(ops.conv2d_first_bwd_filter_workspace_bytes(_dev(x)) // 4, device='cuda')
    runs = []
    for _ in range(2):
        dw2, db3 = torch.zeros((3, 3, cin, 64), device='cuda'), torch.zeros(64, device='cuda')
        ops.conv2d_first_bwd_filter(_dev(x), dya, dw2, db3, workspace=ws)
        torch.cuda.synchronize()
        runs.append((dw2, db3))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    np.testing.assert_allclose(runs[0][0].cpu().numpy(), ref, rtol=1e-4, atol=max(1e-2 * grow, 2e-5 * np.abs(ref).max()))       # (fp32 sums of terms up to 65535 x |dy|)


def test_optimizers_match_tf1_formulas(ops):
    rng = np.random.default_rng(0)
    p0 = rng.standard_normal(1000).astype(np.float32)
    g = rng.standard_normal(1000).astype(np.float32)
    p, m, v = _dev(p0), torch.zeros(1000, device='cuda'), torch.zeros(1000, device='cuda')
    pr, mr, vr = p0.astype(np.float64), np.zeros(1000), np.zeros(1000)
    for t in (1, 2, 3):
        lr_t = 1e-2 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        ops.adam_step(p, _dev(g), m, v, float(lr_t))
        pr, mr, vr = fu.adam_step(pr, g.astype(np.float64), mr, vr, t, lr=1e-2)
    torch.cuda.synchronize()
    np.testing.assert_allclose(p.cpu().numpy(), pr, rtol=1e-5, atol=1e-6)
    p, ms = _dev(p0), torch.ones(1000, device='cuda')
    ops.rmsprop_step(p, _dev(g), ms, 1e-2)
    ref, _ = fu.rmsprop_step(p0.astype(np.float64), g.astype(np.float64), np.ones(1000), lr=1e-2)
    np.testing.assert_allclose(p.cpu().numpy(), ref, rtol=1e-5, atol=1e-6)
    p, acc = _dev(p0), torch.full((1000,), 0.1, device='cuda')
    ops.adagrad_step(p, _dev(g), acc, 1e-2, grad_scale=0.5)
    ref, _ = fu.adagrad_step(p0.astype(np.float64), 0.5 * g.astype(np.float64), np.full(1000, 0.1), lr=1e-2)
    np.testing.assert_allclose(p.cpu().numpy(), ref, rtol=1e-5, atol=1e-6)


def _rel(a, b):
    return np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b) + 1e-30)


def test_training_step_gradients_and_fit(ops, tmp_path):
    from modular_semantic_segmentation_amd import get_model
    C, U, H, W = 12, 64, 32, 48
    rng = np.random.default_rng(0)
    data = {'rgb': rng.integers(0, 256, (2, H, W, 3)).astype(np.float32),
            'labels': rng.integers(-1, C, (2, H, W)).astype(np.int32)}
    w = fo.init_fcn_weights('rgb', 3, U, C, seed=1, bias_scale=0.02)
    w['rgb/conv1_1/kernel'] *= 0.02
    for k in w:
        if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] *= 1.6
    path = str(tmp_path / 'w.npz')
    np.savez(path, **w)
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, C)
    net = get_model('fcn')('rgb', desc, 'rgb', output_dir=str(tmp_path), num_units=U, batch_normalization=False,
                           batchsize=2, learning_rate=1e-3, trainer='adam')
    net.import_weights(path, warnings=False)
    tr = net._ensure_trainer()
    loss = tr.step(_dev(data['rgb']), _dev(data['labels']))
    torch.cuda.synchronize()
    got = tr.grads_as_variables()
    # (1) against autograd over the bf16-policy forward (same relu masks / pool routing): the only
    # difference left is bf16 rounding of the activation gradients and summation order
    ref_loss, ref_g = fo.fcn_loss_and_grads(data['rgb'], data['labels'], w, 'rgb', C, policy='bf16')
    assert abs(loss.item() - ref_loss) < 2e-3 * abs(ref_loss)
    err16 = {name: _rel(got[name], g) for name, g in ref_g.items()}
    # (2) against the fp32 graph the reference differentiates: bf16 storage noise accumulates down the
    # 16-layer backward chain (relu masks / pool arg-maxes flip on near-ties)
    _, ref_g32 = fo.fcn_loss_and_grads(data['rgb'], data['labels'], w, 'rgb', C, policy='fp32')
    err32 = {name: _rel(got[name], g) for name, g in ref_g32.items()}
    print('relative gradient error vs bf16-policy / fp32 oracle:')
    for name in ref_g:
        print('  %-28s %.4f %.4f' % (name, err16[name], err32[name]))
    # Measured on MI355X: 0.2-0.5 % at the head, growing to 5-8 % at the far end of the chain.  The growth
    # is conditioning, not a defect: activation gradients have mixed signs, so every transposed-conv /
    # pooling sum cancels and amplifies the 2^-9 relative rounding of the bf16 gradient tensors (each
    # kernel alone is exact or within bf16 rounding in the tests above).
    assert max(err16.values()) < 0.10, err16
    # which near-tie relu masks flip depends on the last bit of conv1_1: the head figures were 0.3-0.6 % with the FMA
    # first conv and 0.6-1.1 % with the MFMA one (both within fp32 rounding of the exact layer, see
    # test_conv_first_layer_fp32_exactness)
    assert max(v for k, v in err16.items() if k.split('/')[1] in ('score', 'score_conv4')) < 0.02, err16
    assert max(err32.values()) < 0.2, err32
    for name, g in ref_g32.items():
        a, b = got[name].ravel().astype(np.float64), g.ravel().astype(np.float64)
        assert a @ b / (np.linalg.norm(a) * np.linalg.norm(b)) > 0.99, name
    # Adam's first step moves every weight by ~lr against the sign of its gradient (TF1 formula)
    net2 = dict(net.variables)
    tr.to_variables(net2)
    k = 'rgb/conv3_2/kernel'
    moved = net2[k] - w[k]
    big = np.abs(got[k]) > 1e-3 * np.abs(got[k]).max()
    assert (np.sign(moved[big]) == -np.sign(got[k][big])).mean() > 0.999
    # |step| = lr * |g| / (|g| + eps * sqrt(1 - beta2) ... ) -> lr for all but vanishing gradients
    assert (np.abs(np.abs(moved[big]) - 1e-3) < 5e-5).mean() > 0.999
    # fit() runs and lowers the loss on a fixed batch
    first = net._train_batch(data)
    for _ in range(8):
        last = net._train_batch(data)
    assert last < first
    net.fit(data, 2, output=False)
    assert net.global_step == 2
    out = net.export_weights()
    assert np.load(out)['rgb/conv1_1/kernel'].shape == (3, 3, 3, 64)


def test_training_step_with_batch_normalization(ops, tmp_path):
    """`batch_normalization: true` (the reference's example configuration): one step of the batch-norm training graph
    against autograd over the oracle's restatement of it -- loss, gradients of kernels / gamma / beta, moving averages
    ([TF1]: momentum 0.99, unbiased variance); then fit() and inference with the trained statistics.

    Tolerances are calibrated, not guessed: a randomly initialised 16-layer batch-norm network is chaotic with respect
    to bf16 rounding -- perturbing the oracle's own kernels by 3e-7 (fp32 rounding level, i.e. a different summation
    order) moves ITS bf16-policy gradients by 1 % at `score/gamma`, 10 % at `score/kernel` and 25-40 % (cosine
    0.91-0.97) from conv5 down to conv1 (relu masks and pool routes flip on near-ties and every batch statistic
    downstream moves).  The step below sits at exactly that noise floor; every kernel on the path is checked tightly on
    its own in tests/test_batchnorm_gpu.py and the exact-integer conv tests above."""
    from modular_semantic_segmentation_amd import get_model
    from modular_semantic_segmentation_amd.fcn import init_variables
    C, U, H, W = 12, 64, 64, 96
    rng = np.random.default_rng(0)
    data = {'rgb': rng.integers(0, 256, (2, H, W, 3)).astype(np.float32),
            'labels': rng.integers(-1, C, (2, H, W)).astype(np.int32)}
    w = init_variables('rgb', 3, U, C, batch_normalization=True, seed=1)
    for k in w:
        if k.endswith('/gamma'):
            w[k] = rng.uniform(0.8, 1.2, w[k].shape).astype(np.float32)
        elif k.endswith('/beta'):
            w[k] = (0.1 * rng.standard_normal(w[k].shape)).astype(np.float32)
        elif k.endswith('/bias'):
            w[k] = (0.02 * rng.standard_normal(w[k].shape)).astype(np.float32)
    path = str(tmp_path / 'w.npz')
    np.savez(path, **w)
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, C)
    net = get_model('fcn')('rgb', desc, 'rgb', output_dir=str(tmp_path), num_units=U, batch_normalization=True,
                           batchsize=2, learning_rate=1e-3, trainer='adam')
    net.import_weights(path, warnings=False)
    tr = net._ensure_trainer()
    loss = tr.step(_dev(data['rgb']), _dev(data['labels']))
    torch.cuda.synchronize()
    got = tr.grads_as_variables()
    ref_loss, ref_g, stats = fo.fcn_loss_and_grads(data['rgb'], data['labels'], w, 'rgb', C, policy='bf16', batch_norm=True)
    assert abs(loss.item() - ref_loss) < 1e-2 * abs(ref_loss)
    # conv biases in front of a batch norm have an exactly zero gradient (the mean is subtracted): not compared
    names = [k for k in ref_g if not k.endswith('/bias')]
    rel = {k: _rel(got[k], ref_g[k]) for k in names}
    cos = {}
    for k in names:
        a, b = got[k].ravel().astype(np.float64), ref_g[k].ravel().astype(np.float64)
        cos[k] = a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
    print('gradient vs the bf16-policy oracle (batch norm): relative error, cosine')
    for k in sorted(names):
        print('  %-30s %.4f %.4f' % (k, rel[k], cos[k]))
    assert rel['rgb/score/gamma'] < 0.05 and rel['rgb/score/beta'] < 0.08, (rel['rgb/score/gamma'], rel['rgb/score/beta'])
    assert rel['rgb/score/kernel'] < 0.25 and rel['rgb/upscore/gamma'] < 0.25
    assert min(cos.values()) > 0.85, min(cos.items(), key=lambda kv: kv[1])
    assert max(rel.values()) < 0.7, max(rel.items(), key=lambda kv: kv[1])
    # moving averages after one step ([TF1] momentum 0.99; the unbiased batch variance goes into the average)
    out = {}
    tr.to_variables(out)
    for layer in ('conv1_1', 'conv2_1', 'conv3_2', 'score_conv4', 'upscore', 'score'):
        mean, var = stats[layer]
        np.testing.assert_allclose(out['rgb/%s/moving_mean' % layer], 0.99 * w['rgb/%s/moving_mean' % layer] + 0.01 * mean,
                                   rtol=5e-2, atol=5e-3, err_msg=layer)
        np.testing.assert_allclose(out['rgb/%s/moving_variance' % layer],
                                   0.99 * w['rgb/%s/moving_variance' % layer] + 0.01 * var, rtol=5e-2, atol=5e-3,
                                   err_msg=layer)
    # training lowers the loss on a fixed batch, and inference afterwards uses the trained moving statistics
    first = net._train_batch(data)
    for _ in range(10):
        last = net._train_batch(data)
    assert last < first
    label = net.predict(data)
    assert label.shape == (2, H, W) and label.dtype == np.int64
    exported = np.load(net.export_weights())
    assert exported['rgb/conv2_1/moving_variance'].shape == (128,)
    ref = fo.fcn_forward(data['rgb'], {k: exported[k] for k in exported.files}, 'rgb', 'bf16')['score']
    score = net.predict(data, output_attr='score')
    assert np.abs(score - ref).max() < 5e-2 * np.abs(ref).max()


def test_fusion_fcn_training_step(ops, tmp_path):
    """Joint model (fusion_fcn.py:11-40, FusionFCN._build_graph :50-92): one step against autograd over the oracle's
    restatement of the training graph -- loss, every kernel / bias / gamma / beta gradient, the decoder's moving
    averages -- then fit(), export and inference with the trained statistics.

    Tolerances are calibrated like the batch-norm step above: perturbing the oracle's own kernels by 3e-7 moves ITS
    bf16-policy gradients by 0.5-5 % in the decoder head and by 10-19 % (L2) in the fused 1x1 convs and both trunks
    (every gradient passes through the batch statistics of `fused/upscore` at full resolution); the step below sits at
    9-14 % there (cosine 0.99), 0.4-9 % in the head (which summation order the dense head kernels use moves it by that)."""
    from modular_semantic_segmentation_amd import get_model
    C, U, H, W = 12, 64, 32, 48
    prefixes, channels = {'rgb': 'rgb', 'depth': 'depth'}, {'rgb': 3, 'depth': 1}
    rng = np.random.default_rng(0)
    data = {'rgb': rng.integers(0, 256, (2, H, W, 3)).astype(np.float32),
            'depth': rng.integers(0, 65536, (2, H, W, 1)).astype(np.float32),
            'labels': rng.integers(-1, C, (2, H, W)).astype(np.int32)}
    w = fo.init_fusion_fcn_weights(prefixes, channels, U, C, seed=1, bias_scale=0.02)
    w['rgb_conv1_1/kernel'] *= 0.02
    w['depth_conv1_1/kernel'] *= 2e-4
    for k in w:
        if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] *= 1.6
    path = str(tmp_path / 'joint.npz')
    np.savez(path, **w)
    net = get_model('fusion_fcn')(prefixes, channels, U, C, trainer='rmsprop', learning_rate=1e-4,
                                  output_dir=str(tmp_path), batchsize=2)
    net.import_weights(path, warnings=False)
    tr = net._ensure_trainer()
    x = {m: _dev(data[m]) for m in prefixes}
    loss = tr.step(x, _dev(data['labels']))
    torch.cuda.synchronize()
    got = tr.grads_as_variables()
    ref_loss, ref_g, stats = fo.fusion_fcn_loss_and_grads({m: data[m] for m in prefixes}, data['labels'], w, prefixes, C,
                                                          policy='bf16')
    assert abs(loss.item() - ref_loss) < 1e-2 * abs(ref_loss)
    assert set(got) == set(ref_g)
    names = [k for k in ref_g if k != 'fused/score/bias']     # exactly zero: the batch norm subtracts the mean
    rel = {k: _rel(got[k], ref_g[k]) for k in names}
    cos = {}
    for k in names:
        a, b = got[k].ravel().astype(np.float64), ref_g[k].ravel().astype(np.float64)
        cos[k] = a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
    print('joint model: gradient vs the bf16-policy oracle: relative error, cosine')
    for k in sorted(names):
        print('  %-30s %.4f %.4f' % (k, rel[k], cos[k]))
    head = ('fused/score/gamma', 'fused/score/beta', 'fused/score/kernel', 'fused/upscore/gamma', 'fused/upscore/beta')
    assert max(rel[k] for k in head) < 0.12, {k: rel[k] for k in head}      # 1-3x the oracle's own 3e-7 sensitivity there
    assert max(rel.values()) < 0.30, max(rel.items(), key=lambda kv: kv[1])
    assert min(cos.values()) > 0.96, min(cos.items(), key=lambda kv: kv[1])
    out = {}
    tr.to_variables(out)
    for layer in ('fused/upscore', 'fused/score'):
        mean, var = stats[layer]
        np.testing.assert_allclose(out[layer + '/moving_mean'], 0.99 * w[layer + '/moving_mean'] + 0.01 * mean,
                                   rtol=2e-2, atol=2e-3)
        np.testing.assert_allclose(out[layer + '/moving_variance'], 0.99 * w[layer + '/moving_variance'] + 0.01 * var,
                                   rtol=2e-2, atol=2e-3)
    # RMSProp ([TF1]: ms starts at 1): step = -lr * g / sqrt(0.9 + 0.1 g^2 + 1e-10)
    k = 'rgb_conv3_2/kernel'
    g = got[k]
    # (the difference of two float32 weights of size ~0.02 is only known to an ulp, 1.9e-9)
    np.testing.assert_allclose(out[k] - w[k], -1e-4 * g / np.sqrt(0.9 + 0.1 * g * g + 1e-10), rtol=1e-3, atol=4e-9)
    first = net._train_batch(data)
    for _ in range(8):
        last = net._train_batch(data)
    assert last < first
    net.fit(data, 2, output=False)
    assert net.global_step == 2
    pred = net.predict(data)                         # inference engine rebuilt from the trained variables
    assert pred.shape == (2, H, W)
    saved = np.load(net.export_weights())
    assert saved['fused_score_conv4/kernel'].shape == (1, 1, 1024, U) and not np.array_equal(
        saved['fused_score_conv4/kernel'], w['fused_score_conv4/kernel'])
    ref = fo.fusion_fcn_forward({m: data[m] for m in prefixes}, {k: saved[k] for k in saved.files}, prefixes, policy='bf16')
    # (labels on clear margins: a few large steps can leave near-degenerate logits whose argmax is a rounding error away)
    ref_lab = fo.argmax_last(fo.softmax(ref['score']))
    top2 = np.sort(ref['score'], -1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 6e-2 * np.abs(ref['score']).max()
    assert np.array_equal(pred[clear], ref_lab[clear])
    assert (pred == ref_lab).mean() > 0.97 or clear.mean() < 0.5


def test_fusion_fcn_training_with_padded_units(ops, tmp_path):
    """Joint model with num_units = 20, num_classes = 14: the U lanes are padded to 64 inside, variables and gradients
    keep the reference shapes."""
    from modular_semantic_segmentation_amd import get_model
    C, U, H, W = 14, 20, 32, 48
    prefixes, channels = {'rgb': 'rgb', 'depth': 'depth'}, {'rgb': 3, 'depth': 1}
    rng = np.random.default_rng(1)
    data = {'rgb': rng.integers(0, 256, (2, H, W, 3)).astype(np.float32),
            'depth': rng.integers(0, 65536, (2, H, W, 1)).astype(np.float32),
            'labels': rng.integers(-1, C, (2, H, W)).astype(np.int32)}
    w = fo.init_fusion_fcn_weights(prefixes, channels, U, C, seed=3, bias_scale=0.02)
    w['rgb_conv1_1/kernel'] *= 0.02
    w['depth_conv1_1/kernel'] *= 2e-4
    for k in w:
        if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] *= 1.6
    path = str(tmp_path / 'joint20.npz')
    np.savez(path, **w)
    net = get_model('fusion_fcn')(prefixes, channels, U, C, trainer='adam', learning_rate=1e-4, batchsize=2)
    net.import_weights(path, warnings=False)
    tr = net._ensure_trainer()
    loss = tr.step({m: _dev(data[m]) for m in prefixes}, _dev(data['labels']))
    torch.cuda.synchronize()
    ref_loss, ref_g, _ = fo.fusion_fcn_loss_and_grads({m: data[m] for m in prefixes}, data['labels'], w, prefixes, C,
                                                      policy='bf16')
    assert abs(loss.item() - ref_loss) < 1e-2 * abs(ref_loss)
    got = tr.grads_as_variables()
    assert {k: v.shape for k, v in got.items()} == {k: v.shape for k, v in ref_g.items()}
    for k in ('fused/score/gamma', 'fused/score/kernel', 'fused_score_conv5/kernel'):
        assert _rel(got[k], ref_g[k]) < 0.25, (k, _rel(got[k], ref_g[k]))
    out = {}
    tr.to_variables(out)
    assert all(out[k].shape == w[k].shape for k in out)
    assert net.predict(data).shape == (2, H, W)


@pytest.mark.parametrize('kind', ['fcn', 'fcn_bn', 'fusion_fcn'])
def test_filter_gradients_on_their_own_stream_same_bits(ops, tmp_path, monkeypatch, kind):
    """The three trainers run their filter gradients on a second HIP stream (trainer._WGRAD_STREAM): two steps
    with and without it from the same weights and batch -- loss, gradient buffer and parameters bit-identical (a cross-stream
    race on a gradient map, the slab workspace or the join in front of the optimizer would show here, not as a tolerance
    failure against the oracle)."""
    from modular_semantic_segmentation_amd import get_model, trainer
    from modular_semantic_segmentation_amd.fcn import init_variables
    C, U, H, W = 12, 64, 64, 128
    rng = np.random.default_rng(11)
    data = {'rgb': rng.integers(0, 256, (2, H, W, 3)).astype(np.float32),
            'depth': rng.integers(0, 65536, (2, H, W, 1)).astype(np.float32),
            'labels': rng.integers(-1, C, (2, H, W)).astype(np.int32)}
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, C)
    path = str(tmp_path / 'w.npz')
    if kind == 'fusion_fcn':
        prefixes, channels = {'rgb': 'rgb', 'depth': 'depth'}, {'rgb': 3, 'depth': 1}
        w = fo.init_fusion_fcn_weights(prefixes, channels, U, C, seed=3, bias_scale=0.02)
        w['rgb_conv1_1/kernel'] *= 0.02
        w['depth_conv1_1/kernel'] *= 2e-4
    else:
        w = init_variables('rgb', 3, U, C, batch_normalization=kind == 'fcn_bn', seed=3)
        w['rgb/conv1_1/kernel'] *= 0.02
    np.savez(path, **w)
    results = []
    for second_stream in (True, False):
        monkeypatch.setattr(trainer, '_WGRAD_STREAM', second_stream)
        if kind == 'fusion_fcn':
            net = get_model('fusion_fcn')(prefixes, channels, U, C, trainer='rmsprop', learning_rate=1e-4,
                                          output_dir=str(tmp_path), batchsize=2)
            x = {m: _dev(data[m]) for m in prefixes}
        else:
            net = get_model('fcn')('rgb', desc, 'rgb', output_dir=str(tmp_path), num_units=U,
                                   batch_normalization=kind == 'fcn_bn', batchsize=2, learning_rate=1e-3, trainer='adam')
            x = _dev(data['rgb'])
        net.import_weights(path, warnings=False)
        tr = net._ensure_trainer()
        losses = [tr.step(x, _dev(data['labels'])).item() for _ in range(2)]
        torch.cuda.synchronize()
        results.append((losses, tr.grad.clone(), tr.param.clone()))
    assert results[0][0] == results[1][0]
    assert torch.equal(results[0][1], results[1][1])
    assert torch.equal(results[0][2], results[1][2])


@pytest.mark.parametrize('kind', ['fcn_bn', 'fusion_fcn'])
def test_batch_norm_behind_the_x8_deconv_without_its_input_in_memory(ops, tmp_path, monkeypatch, kind):
    """The batch-norm and joint trainers recompute the x8 deconv's output in the four batch-norm passes that would read it
    back (xv_bn_*_ups8, trainer._VIRTUAL_UPSCORE) instead of storing 0.6 GB: the same values element by element (one
    bilinear fmaf chain and rounding in every caller), the statistics and gradient sums over them added in another fixed
    order -- so a step with and one without agree to fp32 summation order (each is bitwise reproducible by itself:
    tools/stress_train_step.py)."""
    from modular_semantic_segmentation_amd import get_model, trainer
    from modular_semantic_segmentation_amd.fcn import init_variables
    C, U, H, W = 12, 64, 64, 96
    rng = np.random.default_rng(12)
    data = {'rgb': rng.integers(0, 256, (2, H, W, 3)).astype(np.float32),
            'depth': rng.integers(0, 65536, (2, H, W, 1)).astype(np.float32),
            'labels': rng.integers(-1, C, (2, H, W)).astype(np.int32)}
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, C)
    path = str(tmp_path / 'w.npz')
    if kind == 'fusion_fcn':
        prefixes, channels = {'rgb': 'rgb', 'depth': 'depth'}, {'rgb': 3, 'depth': 1}
        w = fo.init_fusion_fcn_weights(prefixes, channels, U, C, seed=4, bias_scale=0.02)
        w['rgb_conv1_1/kernel'] *= 0.02
        w['depth_conv1_1/kernel'] *= 2e-4
    else:
        w = init_variables('rgb', 3, U, C, batch_normalization=True, seed=4)
        w['rgb/conv1_1/kernel'] *= 0.02
    np.savez(path, **w)
    results = []
    for virtual in (True, False):
        monkeypatch.setattr(trainer, '_VIRTUAL_UPSCORE', virtual)
        if kind == 'fusion_fcn':
            net = get_model('fusion_fcn')(prefixes, channels, U, C, trainer='rmsprop', learning_rate=1e-4,
                                          output_dir=str(tmp_path), batchsize=2)
            x = {m: _dev(data[m]) for m in prefixes}
        else:
            net = get_model('fcn')('rgb', desc, 'rgb', output_dir=str(tmp_path), num_units=U, batch_normalization=True,
                                   batchsize=2, learning_rate=1e-3, trainer='adam')
            x = _dev(data['rgb'])
        net.import_weights(path, warnings=False)
        tr = net._ensure_trainer()
        l1 = tr.step(x, _dev(data['labels'])).item()
        g1 = tr.grad.clone()
        l2 = tr.step(x, _dev(data['labels'])).item()
        torch.cuda.synchronize()
        results.append(((l1, l2), g1, tr.param.clone()))
    (la, ga, pa), (lb, gb, pb) = results
    assert abs(la[0] - lb[0]) <= 1e-6 * abs(lb[0]) and abs(la[1] - lb[1]) <= 1e-3 * abs(lb[1])
    # the gradients of the first step: the same terms added in another order (fp32 partial sums), amplified along the
    # backward chain through 16 batch norms
    assert (ga - gb).norm().item() <= 2e-3 * gb.norm().item()
