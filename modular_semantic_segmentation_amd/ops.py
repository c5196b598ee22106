"""Thin torch-tensor wrappers over the C ABI (pointers + sizes in, nothing else).

PyTorch is plumbing here: it owns device memory and the stream; every arithmetic op of the
hot path runs in libxview_hip.so.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import xv_act


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _need(t, dtype, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TypeError('%s must be a contiguous CUDA tensor of dtype %s' % (name, dtype))


BF16, FP8 = _lib.CONSTANTS['XV_BF16'], _lib.CONSTANTS['XV_FP8']            # xv_act.dtype (include/xview_hip.h)
XV_ESHAPE = _lib.CONSTANTS['XV_ESHAPE']
FP8_MAX = 448.0             # largest finite OCP e4m3fn


class Act(object):
    """padded-NHWC activation (include/xview_hip.h `xv_act`): dense [n][h+2][w+2][c] with a zero 1-pixel border
    that no kernel ever writes.  dtype 'bf16' (default) or 'fp8' (OCP e4m3fn bytes; a stored q stands for
    q * 2**scale_exp -- the forward convolutions' fp8 path)."""

    def __init__(self, n, h, w, c, device='cuda', dtype='bf16', scale_exp=0):
        self.n, self.h, self.w, self.c = int(n), int(h), int(w), int(c)
        self.dtype, self.scale_exp = dtype, int(scale_exp)
        tdt = torch.bfloat16 if dtype == 'bf16' else torch.float8_e4m3fn
        self.t = torch.zeros((self.n, self.h + 2, self.w + 2, self.c), dtype=tdt, device=device)
        self._xv = xv_act(self.t.data_ptr(), self.n, self.h, self.w, self.c, BF16 if dtype == 'bf16' else FP8,
                          self.scale_exp)

    def xv(self):
        return ctypes.byref(self._xv)

    def set_scale_exp(self, scale_exp):
        self.scale_exp = self._xv.scale_exp = int(scale_exp)

    def interior(self):
        """Logical [n][h][w][c] view (storage dtype)."""
        return self.t[:, 1:-1, 1:-1, :]

    def real(self):
        """Interior as float32 in real units (test / calibration helper)."""
        v = self.interior().float()
        return v * (2.0 ** self.scale_exp) if self.dtype == 'fp8' else v

    def images(self, n0, n1):
        """Images n0 .. n1-1 as an Act sharing this one's storage (a slot of a slot-major batch)."""
        v = Act.__new__(Act)
        v.n, v.h, v.w, v.c, v.dtype, v.scale_exp = int(n1) - int(n0), self.h, self.w, self.c, self.dtype, self.scale_exp
        v.t = self.t[int(n0):int(n1)]
        v._xv = xv_act(v.t.data_ptr(), v.n, v.h, v.w, v.c, self._xv.dtype, self.scale_exp)
        return v

    @classmethod
    def from_dense(cls, x, dtype='bf16', scale_exp=0):
        """Test helper: pad a dense NHWC float tensor into a new Act (rounds to the storage dtype; fp8 stores
        x / 2**scale_exp, saturating)."""
        n, h, w, c = x.shape
        a = cls(n, h, w, c, device=x.device, dtype=dtype, scale_exp=scale_exp)
        if dtype == 'bf16':
            a.interior().copy_(x.to(torch.bfloat16))
        else:
            a.interior().copy_((x.float() * (2.0 ** -scale_exp)).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn))
        return a


def fp8_scale_exp(amax, margin_bits=0):
    """Smallest power-of-two exponent e with amax / 2**e <= 448 (plus `margin_bits` of headroom)."""
    import math
    amax = float(amax)
    if not amax > 0:
        return 0
    return int(math.ceil(math.log2(amax / FP8_MAX))) + int(margin_bits)


def fp8_scale_exp_mse(values, margin_bits=0, search=6, max_elems=1 << 24):
    """The power-of-two exponent e that minimises the squared error of `values` (a device tensor) stored as e4m3 of
    value / 2**e, saturating at +-448: between the exponent that fits the largest magnitude (+ margin_bits) and `search`
    below it.  A map whose magnitudes have a long tail (the depth expert: raw uint16 depth, logit scale 360) keeps three
    mantissa bits for its bulk instead of spending the format's range on a few outliers, which then saturate.  Calibration
    time only (torch ops on a strided sample of at most max_elems values)."""
    v = values.reshape(-1)
    if v.numel() > max_elems:
        v = v[::(v.numel() + max_elems - 1) // max_elems]
    v = v.float()
    amax = float(v.abs().max())
    if not amax > 0:
        return 0
    top = fp8_scale_exp(amax, margin_bits)
    best, best_err = top, None
    for e in range(top, top - search - 1, -1):
        q = (v * (2.0 ** -e)).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).float() * (2.0 ** e)
        err = float(((q - v) ** 2).sum())
        if best_err is None or err < best_err:
            best, best_err = e, err
    return best


_NULL_ACT = ctypes.POINTER(xv_act)()

# bench.py sets this to a list to collect (kind, flops, start_event, end_event) per MFMA-conv launch;
# the events are recorded on the stream the kernel is launched on.
CONV_PROFILE = None


def packed_weight_elems(k, cin, cout):
    """bf16 elements of the packed weight buffer of a k x k conv (3x3: three images, see xview_hip.h)."""
    return _lib.lib().xv_packed_weight_bytes(k, cin, cout) // 2


def pack_conv_weights(w_hwio):
    """float32 HWIO device tensor -> packed bf16 weight buffer for conv2d_fwd."""
    _need(w_hwio, torch.float32, 'w_hwio')
    k, k2, cin, cout = w_hwio.shape
    nbytes = _lib.lib().xv_packed_weight_bytes(k, cin, cout)
    if k != k2 or nbytes == 0:
        raise _lib.XvError('unsupported conv weight shape %s' % (tuple(w_hwio.shape),))
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w_hwio.device)
    _lib.check(_lib.lib().xv_pack_conv_weights(_ptr(w_hwio), _ptr(out), k, cin, cout, _stream()), 'xv_pack_conv_weights')
    return out


def pack_conv_weights_f8(w_hwio, scale_exp=None):
    """float32 HWIO device tensor -> (packed e4m3 weight buffer with its scale-exponent header, exponent); the
    exponent defaults to the smallest one that keeps max|w| finite."""
    _need(w_hwio, torch.float32, 'w_hwio')
    k, k2, cin, cout = w_hwio.shape
    nbytes = _lib.lib().xv_packed_weight_bytes_f8(k, cin, cout)
    if k != k2 or nbytes == 0:
        raise _lib.XvError('unsupported fp8 conv weight shape %s' % (tuple(w_hwio.shape),))
    if scale_exp is None:
        scale_exp = fp8_scale_exp(w_hwio.abs().max().item())        # one-off, at load time
    out = torch.empty(nbytes, dtype=torch.uint8, device=w_hwio.device)
    _lib.check(_lib.lib().xv_pack_conv_weights_f8(_ptr(w_hwio), _ptr(out), k, cin, cout, int(scale_exp), _stream()),
               'xv_pack_conv_weights_f8')
    return out, int(scale_exp)


def streamk_workspace(device):
    """A zeroed stream-K workspace (xv_conv2d_streamk_workspace_bytes): hand it to every conv2d_fwd / conv2d_bwd_data of
    ONE stream; two streams (the two experts of a fusion model) need one each."""
    return torch.zeros(_lib.lib().xv_conv2d_streamk_workspace_bytes(), dtype=torch.uint8, device=device)


def split_workspace(x, cout, arena, key='split_ws'):
    """The fp32 slab workspace of the split form for a 3x3 conv of Act x onto `cout` channels (xv_conv2d_split_workspace_bytes),
    kept in the caller's `arena` dict under `key` and grown as needed; None where this shape / batch is never split.  One per
    stream: the launch owns it until it has completed."""
    need = _lib.lib().xv_conv2d_split_workspace_bytes(x.n, x.h, x.w, x.c, cout)
    if need == 0:
        return None
    ws = arena.get(key)
    if ws is None or ws.numel() * 4 < need:
        ws = arena[key] = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.t.device)
    return ws


def conv2d_fwd(x, w_packed, bias, k, relu=True, y=None, pooled=None, write_y=True, cfg=-1, workspace=None, split_ws=None):
    """x: Act; returns (y Act or None, pooled Act or None).  An fp8 `x` needs weights from pack_conv_weights_f8; the
    dtype / scale of y and pooled (which must agree) select the output conversion.  workspace (streamk_workspace): the
    generation-2 kernel deals the items of an incomplete last round of tiles out over all CUs (stream-K tail).  split_ws
    (split_workspace): layers whose tiles fill less than half the CUs run in the split form of the 24x16-tile kernel (batch-1
    latency; the same bits as the unsplit launch)."""
    cout = bias.numel()
    _need(bias, torch.float32, 'bias')
    if y is None and write_y:
        y = Act(x.n, x.h, x.w, cout, x.t.device)
    if y is not None:
        ydesc = y._xv
    else:   # pooled-only: the descriptor still names the output dtype
        ydesc = xv_act(None, x.n, x.h, x.w, cout, pooled._xv.dtype, pooled._xv.scale_exp)
    prof = CONV_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    if workspace is None and split_ws is not None:
        rc = _lib.lib().xv_conv2d_fwd_split(x.xv(), _ptr(w_packed), _ptr(bias), ctypes.byref(ydesc),
                                           pooled.xv() if pooled is not None else _NULL_ACT, k, int(bool(relu)), int(cfg),
                                           _ptr(split_ws), split_ws.numel() * split_ws.element_size(), _stream())
    elif workspace is None:
        rc = _lib.lib().xv_conv2d_fwd_cfg(x.xv(), _ptr(w_packed), _ptr(bias), ctypes.byref(ydesc),
                                         pooled.xv() if pooled is not None else _NULL_ACT, k, int(bool(relu)), int(cfg),
                                         _stream())
    else:
        rc = _lib.lib().xv_conv2d_fwd_ws(x.xv(), _ptr(w_packed), _ptr(bias), ctypes.byref(ydesc),
                                        pooled.xv() if pooled is not None else _NULL_ACT, k, int(bool(relu)), int(cfg),
                                        _ptr(workspace), workspace.numel() * workspace.element_size(), _stream())
    _lib.check(rc, 'xv_conv2d_fwd')
    if prof is not None:
        ev1.record()
        prof.append(('k%d%s' % (k, 'f8' if x.dtype == 'fp8' else ''),
                     2.0 * x.n * x.h * x.w * x.c * cout * k * k, ev0, ev1))
    return y, pooled


def conv2d_fwd_pair(xa, wa, ba, xb, wb, bb, relu=True, ya=None, yb=None, pa=None, pb=None):
    """The same 3x3 layer of two models in ONE launch (xv_conv2d_fwd_pair): per model the arguments of conv2d_fwd; the
    outputs wanted (full maps ya / yb, pooled maps pa / pb) must be given and be the same set for both.  Returns False --
    nothing launched -- where the shape does not run on the generation-4 / 5 kernels: the caller launches two conv2d_fwd."""
    _need(ba, torch.float32, 'bias_a')
    _need(bb, torch.float32, 'bias_b')
    cout = ba.numel()
    if xa.dtype != 'bf16' or xb.dtype != 'bf16' or (ya is None) != (yb is None) or (pa is None) != (pb is None) or \
            (ya is None and pa is None):
        return False

    def desc(y, x, p):
        return y._xv if y is not None else xv_act(None, x.n, x.h, x.w, cout, p._xv.dtype, p._xv.scale_exp)
    da, db = desc(ya, xa, pa), desc(yb, xb, pb)
    prof = CONV_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    rc = _lib.lib().xv_conv2d_fwd_pair(xa.xv(), _ptr(wa), _ptr(ba), ctypes.byref(da), pa.xv() if pa is not None else _NULL_ACT,
                                       xb.xv(), _ptr(wb), _ptr(bb), ctypes.byref(db), pb.xv() if pb is not None else _NULL_ACT,
                                       int(bool(relu)), _stream())
    if rc == XV_ESHAPE:
        return False
    _lib.check(rc, 'xv_conv2d_fwd_pair')
    if prof is not None:
        ev1.record()
        prof.append(('k3', 2.0 * 2 * xa.n * xa.h * xa.w * xa.c * cout * 9, ev0, ev1))
    return True


def conv2d_first_fwd(x, w_hwio, bias, y, relu=True):
    _need(x, torch.float32, 'x')
    _need(w_hwio, torch.float32, 'w_hwio')
    _need(bias, torch.float32, 'bias')
    n, h, w, cin = x.shape
    rc = _lib.lib().xv_conv2d_first_fwd(_ptr(x), n, h, w, cin, _ptr(w_hwio), _ptr(bias), y.xv(), int(bool(relu)), _stream())
    _lib.check(rc, 'xv_conv2d_first_fwd')
    return y


def conv2d_first_gather7s2_fwd(x, w_hwio, bias, z, relu=True):
    """relu(conv3x3(x) + b) of the raw input written directly as gather_conv7s2's operand z [N,H/2,W/2,576] (z must hold
    zeros where the gather has no source pixel: a fresh Act, or one only ever written by this op / gather_conv7s2)."""
    _need(x, torch.float32, 'x')
    _need(w_hwio, torch.float32, 'w_hwio')
    _need(bias, torch.float32, 'bias')
    n, h, w, cin = x.shape
    rc = _lib.lib().xv_conv2d_first_gather7s2_fwd(_ptr(x), n, h, w, cin, _ptr(w_hwio), _ptr(bias), z.xv(), int(bool(relu)),
                                                  _stream())
    _lib.check(rc, 'xv_conv2d_first_gather7s2_fwd')
    return z


def conv_first_pair_fwd(x, w1_hwio, b1, w2_packed, b2, y=None, pooled=None, relu1=True, relu2=True):
    """conv1_1 + conv1_2 (+ pool) in one launch (xv_conv_first_pair_fwd): x raw float32 NHWC, y / pooled bf16 Acts (either
    may be None).  Returns False -- nothing launched -- where the fused kernel does not apply (maps that do not tile in
    16x32, other channel counts): the caller then runs conv2d_first_fwd + conv2d_fwd."""
    _need(x, torch.float32, 'x')
    _need(w1_hwio, torch.float32, 'w1_hwio')
    n, h, w, cin = x.shape
    if cin not in (1, 3) or h % 16 or w % 32 or (y is None and pooled is None):
        return False
    prof = CONV_PROFILE
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    rc = _lib.lib().xv_conv_first_pair_fwd(_ptr(x), n, h, w, cin, _ptr(w1_hwio), _ptr(b1), int(bool(relu1)), _ptr(w2_packed),
                                           _ptr(b2), int(bool(relu2)), y.xv() if y is not None else _NULL_ACT,
                                           pooled.xv() if pooled is not None else _NULL_ACT, _stream())
    if rc == XV_ESHAPE:
        return False
    _lib.check(rc, 'xv_conv_first_pair_fwd')
    if prof is not None:
        # bench.py: a kind of its own (not the plain 3x3 conv kernel the roofline record is about), with the algorithmic FLOPs
        # of BOTH layers; conv1_1's recomputation on the halo and its three-way operand split count as time, not as FLOPs
        ev1.record()
        prof.append(('k3pair', 2.0 * n * h * w * 64 * 9 * (cin + 64), ev0, ev1))
    return True


def maxpool2x2_fwd(x, y=None):
    if y is None:
        y = Act(x.n, x.h // 2, x.w // 2, x.c, x.t.device)
    _lib.check(_lib.lib().xv_maxpool2x2_fwd(x.xv(), y.xv(), _stream()), 'xv_maxpool2x2_fwd')
    return y


def upsample2x_relu_add(x, residual=None, y=None, scale=None, shift=None, relu=True):
    """y = act(bilinear_x2(x) [* scale + shift]) [+ residual]; scale / shift: float32 [C] inference batch norm."""
    if y is None:
        y = Act(x.n, 2 * x.h, 2 * x.w, x.c, x.t.device)
    if scale is not None:
        _need(scale, torch.float32, 'scale')
        _need(shift, torch.float32, 'shift')
    rc = _lib.lib().xv_upsample2x_affine_act_add(x.xv(), _ptr(scale), _ptr(shift),
                                                residual.xv() if residual is not None else _NULL_ACT, y.xv(),
                                                int(bool(relu)), _stream())
    _lib.check(rc, 'xv_upsample2x_affine_act_add')
    return y


def deconv_dense_fwd(x, w_phases_packed, zero_bias, stride, cout, y=None, scale=None, shift=None, residual=None,
                     relu=True, workspace=None):
    """y = act(conv2d_transpose(x, W) [* scale + shift]) [+ residual] for an arbitrary kernel with k = 2 * stride
    (w_phases_packed: pack_conv_weights(dense_deconv_as_conv3x3(W, stride))).  Returns (y, workspace)."""
    if y is None:
        y = Act(x.n, x.h * stride, x.w * stride, cout, x.t.device)
    need = _lib.lib().xv_deconv_dense_workspace_bytes(x.n, x.h, x.w, cout, stride)
    if workspace is None or workspace.numel() * 2 < need:
        workspace = torch.zeros(need // 2, dtype=torch.bfloat16, device=x.t.device)
    rc = _lib.lib().xv_deconv_dense_fwd(x.xv(), _ptr(w_phases_packed), _ptr(zero_bias), _ptr(scale), _ptr(shift),
                                       residual.xv() if residual is not None else _NULL_ACT, y.xv(), int(stride),
                                       int(bool(relu)), _ptr(workspace), workspace.numel() * 2, _stream())
    _lib.check(rc, 'xv_deconv_dense_fwd')
    return y, workspace


def conv1x1_residual(x, w_packed, bias, residual, relu=True, y=None):
    """y = act(conv1x1(x) + bias) + residual (the closing conv of a ResNet block)."""
    _need(bias, torch.float32, 'bias')
    if y is None:
        y = Act(x.n, x.h, x.w, bias.numel(), x.t.device)
    rc = _lib.lib().xv_conv2d_fwd_residual(x.xv(), _ptr(w_packed), _ptr(bias), residual.xv(), y.xv(), int(bool(relu)),
                                          _stream())
    _lib.check(rc, 'xv_conv2d_fwd_residual')
    return y


def subsample2(x, y=None):
    """y[i][j] = x[2i][2j]."""
    if y is None:
        y = Act(x.n, x.h // 2, x.w // 2, x.c, x.t.device)
    _lib.check(_lib.lib().xv_subsample2(x.xv(), y.xv(), _stream()), 'xv_subsample2')
    return y


def gather_conv7s2(x, z=None):
    """[N,H/2,W/2,9C] operand that turns a 7x7 stride-2 'same' conv into a 3x3 stride-1 one (see pack_conv7s2)."""
    if z is None:
        z = Act(x.n, x.h // 2, x.w // 2, 9 * x.c, x.t.device)
    _lib.check(_lib.lib().xv_gather_conv7s2(x.xv(), z.xv(), _stream()), 'xv_gather_conv7s2')
    return z


def subsample2_bwd(dy, dx):
    _lib.check(_lib.lib().xv_subsample2_bwd(dy.xv(), dx.xv(), _stream()), 'xv_subsample2_bwd')
    return dx


def gather_conv7s2_bwd(dz, dx):
    _lib.check(_lib.lib().xv_gather_conv7s2_bwd(dz.xv(), dx.xv(), _stream()), 'xv_gather_conv7s2_bwd')
    return dx


def im2col_dilated_pair_bwd(dz, d1, d2, dx):
    _lib.check(_lib.lib().xv_im2col_dilated_pair_bwd(dz.xv(), int(d1), int(d2), dx.xv(), _stream()),
               'xv_im2col_dilated_pair_bwd')
    return dx


def add(a, b, y=None):
    """y = a + b (Acts of one shape)."""
    if y is None:
        y = Act(a.n, a.h, a.w, a.c, a.t.device)
    _lib.check(_lib.lib().xv_add(a.xv(), b.xv(), y.xv(), _stream()), 'xv_add')
    return y


def space_to_depth(g, stride, out=None):
    """[N,s*H,s*W,C] Act -> [N,H,W,s*s*C] Act, phase channel (py*s + px)*C + c (gradient side of a dense deconv)."""
    if out is None:
        out = Act(g.n, g.h // stride, g.w // stride, stride * stride * g.c, g.t.device)
    _lib.check(_lib.lib().xv_space_to_depth(g.xv(), int(stride), out.xv(), _stream()), 'xv_space_to_depth')
    return out


def space_to_depth_dense(g, stride, out):
    """dense float32 [N,s*H,s*W,C] -> Act [N,H,W,s*s*Cp] (Cp = out.c / s^2 >= C, padding channels zero)."""
    _need(g, torch.float32, 'g')
    _lib.check(_lib.lib().xv_space_to_depth_dense(_ptr(g), int(g.shape[-1]), int(stride), out.xv(), _stream()),
               'xv_space_to_depth_dense')
    return out


def depth_to_space_dense(z, stride, num_classes, out, scale=None, shift=None):
    """phase map Act [N,H,W,s*s*Cp] -> dense float32 [N,s*H,s*W,C] [* scale + shift]."""
    _need(out, torch.float32, 'out')
    if scale is not None:
        _need(scale, torch.float32, 'scale')
        _need(shift, torch.float32, 'shift')
    rc = _lib.lib().xv_depth_to_space_dense(z.xv(), int(stride), int(num_classes), _ptr(scale), _ptr(shift), _ptr(out),
                                            _stream())
    _lib.check(rc, 'xv_depth_to_space_dense')
    return out


def deconv8_scores_f32(x, w_hwio_f32, num_classes, cp, out, arena, scale=None, shift=None):
    """AdapNet's trained x8 score deconv in float32: the padded bf16 map `x` as dense float32 (exact), its 3x3 conv onto the 64
    phases x cp classes (w_hwio_f32 = dense_deconv_as_conv3x3(kernel, 8), float32 [3,3,U,64*cp]) on the fp32 matrix
    instruction, the phases unshuffled into the dense float32 scores `out` [N,8H,8W,C] [* scale + shift].  The scores never
    pass through bf16 (adapnet.py:155-163).  arena: dict for the two float32 scratch maps."""
    _need(out, torch.float32, 'out')
    _need(w_hwio_f32, torch.float32, 'w_hwio_f32')
    lib = _lib.lib()
    xd = arena.get(('d8_x', x.n, x.h, x.w, x.c))
    if xd is None:
        xd = arena[('d8_x', x.n, x.h, x.w, x.c)] = torch.empty((x.n, x.h, x.w, x.c), dtype=torch.float32, device=x.t.device)
    ph = arena.get(('d8_ph', x.n, x.h, x.w, cp))
    if ph is None:
        ph = arena[('d8_ph', x.n, x.h, x.w, cp)] = torch.empty((x.n, x.h, x.w, 64 * cp), dtype=torch.float32, device=x.t.device)
        arena['d8_zero_bias'] = torch.zeros(64 * cp, dtype=torch.float32, device=x.t.device)
    _lib.check(lib.xv_act_to_dense_f32(x.xv(), _ptr(xd), _stream()), 'xv_act_to_dense_f32')
    _lib.check(lib.xv_conv2d_f32(_ptr(xd), x.n, x.h, x.w, x.c, _ptr(w_hwio_f32), _ptr(arena['d8_zero_bias']), 3, 64 * cp, 0,
                                 _ptr(ph), _stream()), 'xv_conv2d_f32')
    _lib.check(lib.xv_depth_to_space_dense_f32(_ptr(ph), x.n, x.h, x.w, 8, cp, num_classes, _ptr(scale), _ptr(shift), _ptr(out),
                                               _stream()), 'xv_depth_to_space_dense_f32')
    return out


def im2col_dilated_pair(x, d1, d2, z=None):
    """[N,H,W,18C]: the nine taps at dilation d1 then the nine at d2."""
    if z is None:
        z = Act(x.n, x.h, x.w, 18 * x.c, x.t.device)
    _lib.check(_lib.lib().xv_im2col_dilated_pair(x.xv(), int(d1), int(d2), z.xv(), _stream()), 'xv_im2col_dilated_pair')
    return z


def dilated_pair_implicit_ok(cin, cout):
    """Shapes xv_conv_dilated_pair_fwd takes: 64-channel K steps; each 128-channel output block inside one half, or one
    64-channel tile for both."""
    return cin % 64 == 0 and (cout % 256 == 0 or cout == 64)


def conv_dilated_pair(x, w_packed, bias, d1, d2, relu=True, y=None):
    """concat(atrous3x3(x, d1), atrous3x3(x, d2)) [+ relu] without the 18C operand (adapnet.py:84-88); w_packed / bias as the
    1x1 conv over im2col_dilated_pair(x) takes them (adapnet.dilated_pair_as_1x1).  Same bits as that pair of calls."""
    _need(bias, torch.float32, 'bias')
    if y is None:
        y = Act(x.n, x.h, x.w, bias.numel(), x.t.device)
    _lib.check(_lib.lib().xv_conv_dilated_pair_fwd(x.xv(), _ptr(w_packed), _ptr(bias), int(d1), int(d2), int(bool(relu)),
                                                   y.xv(), _stream()), 'xv_conv_dilated_pair_fwd')
    return y


def dilated_pair_training_ok(x, cout):
    """Shapes both gradient entries of the implicit pair take (xv_conv_dilated_pair_bwd_data / _bwd_filter_ws)."""
    return x.c % 256 == 0 and cout % 256 == 0 and \
        _lib.lib().xv_conv_dilated_pair_bwd_filter_workspace_bytes(x.n, x.h, x.w, x.c, cout) > 0


def dilated_pair_dgrad_kernel(kernel1, kernel2, out=None):
    """float32 [1,1,18 F/2,C] kernel of the pair's data gradient as a 1x1 conv over (conv, tap, output channel of the conv): row
    (h * 9 + t) * F/2 + co = k_h[t][:, co].  kernel1 / kernel2: [3,3,C,F/2] device tensors; `out`: a tensor to fill in place."""
    _, _, c, half = kernel1.shape
    if out is None:
        out = torch.empty(1, 1, 18 * half, c, dtype=torch.float32, device=kernel1.device)
    v = out.view(2, 9, half, c)
    v[0].copy_(kernel1.reshape(9, c, half).transpose(1, 2))
    v[1].copy_(kernel2.reshape(9, c, half).transpose(1, 2))
    return out


def conv_dilated_pair_bwd_data(dy, w_packed_dgrad, zero_bias, d1, d2, dx):
    """dx = gradient of the pair's input (xv_conv_dilated_pair_bwd_data); w_packed_dgrad: pack_conv_weights of
    dilated_pair_dgrad_kernel(k1, k2)."""
    with _Profiled('dgrad_pair', 2.0 * dy.n * dy.h * dy.w * dx.c * dy.c * 9):
        rc = _lib.lib().xv_conv_dilated_pair_bwd_data(dy.xv(), _ptr(w_packed_dgrad), _ptr(zero_bias), int(d1), int(d2), dx.xv(),
                                                      _stream())
    _lib.check(rc, 'xv_conv_dilated_pair_bwd_data')
    return dx


def conv_dilated_pair_bwd_filter_workspace_bytes(x, cout):
    return _lib.lib().xv_conv_dilated_pair_bwd_filter_workspace_bytes(x.n, x.h, x.w, x.c, cout)


def conv_dilated_pair_bwd_filter(x, dy, d1, d2, dw1, dw2, workspace):
    """dw1 / dw2 (+=): HWIO [3,3,C,F/2] gradients of the two atrous kernels, without the im2col operand."""
    _need(dw1, torch.float32, 'dw1')
    _need(dw2, torch.float32, 'dw2')
    with _Profiled('wgrad_pair', 2.0 * x.n * x.h * x.w * x.c * dy.c * 9):
        rc = _lib.lib().xv_conv_dilated_pair_bwd_filter_ws(x.xv(), dy.xv(), int(d1), int(d2), _ptr(dw1), _ptr(dw2), _ptr(workspace),
                                                           workspace.numel() * 4, _stream())
    _lib.check(rc, 'xv_conv_dilated_pair_bwd_filter_ws')


def dropout(x, rate, seed, y=None):
    """tf.layers.dropout(x, rate, training=True): keep with probability 1 - rate, scale by 1 / (1 - rate)."""
    if y is None:
        y = Act(x.n, x.h, x.w, x.c, x.t.device)
    _lib.check(_lib.lib().xv_dropout(x.xv(), y.xv(), float(rate), int(seed) & 0xffffffffffffffff, _stream()), 'xv_dropout')
    return y


def dropout_samples(x, num_samples, rate, seed0, stride, y=None, in_place=False, sample_only=False):
    """MC-dropout samples of x (xv_dropout_samples): an Act of (num_samples + 1) * x.n images, slot-major -- slot 0 = x, slot t
    = dropout(x, rate, seed0 + (t - 1) * stride).  in_place=True: x already holds the slots; drop slots 1.. of it (slot 0
    untouched) and return x.  sample_only=True (xv_dropout_samples_only): no plain slot -- num_samples * x.n images, slot t =
    dropout(x, rate, seed0 + t * stride), t = 0 .. num_samples-1; in place every slot of x is dropped."""
    T = int(num_samples)
    seed0, stride = int(seed0) & 0xffffffffffffffff, int(stride) & 0xffffffffffffffff
    name = 'xv_dropout_samples_only' if sample_only else 'xv_dropout_samples'
    if in_place:
        _lib.check(getattr(_lib.lib(), name + '_inplace')(x.xv(), T, float(rate), seed0, stride, _stream()), name + '_inplace')
        return x
    if y is None:
        y = Act((T if sample_only else T + 1) * x.n, x.h, x.w, x.c, x.t.device)
    _lib.check(getattr(_lib.lib(), name)(x.xv(), y.xv(), T, float(rate), seed0, stride, _stream()), name)
    return y


def concat_channels(a, b, y=None):
    if y is None:
        y = Act(a.n, a.h, a.w, a.c + b.c, a.t.device)
    _lib.check(_lib.lib().xv_concat_channels(a.xv(), b.xv(), y.xv(), _stream()), 'xv_concat_channels')
    return y


_HEAD_WS = {}


def _head_workspace(fused, num_classes):
    key = (fused.t.device, fused.n, fused.h, fused.w, num_classes)
    ws = _HEAD_WS.get(key)
    if ws is None:
        nbytes = _lib.lib().xv_decoder_head_workspace_bytes(fused.n, fused.h, fused.w, num_classes)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=fused.t.device)
        _HEAD_WS[key] = ws
    return ws


def decoder_head_fwd(fused, w_score, b_score, num_classes, want_score=False, want_prob=False, want_label=True,
                     out=None, workspace=None, scale=None, shift=None):
    """Returns dict with the requested dense outputs (score/prob float32 NHWC, label int64 NHW).
    scale / shift (float32 [U]): batch norm between the x8 deconv and its relu -> the general (un-commuted) head."""
    _need(w_score, torch.float32, 'w_score')
    _need(b_score, torch.float32, 'b_score')
    dev = fused.t.device
    n, ho, wo = fused.n, fused.h * 8, fused.w * 8
    out = {} if out is None else out
    if want_score and 'score' not in out:
        out['score'] = torch.empty((n, ho, wo, num_classes), dtype=torch.float32, device=dev)
    if want_prob and 'prob' not in out:
        out['prob'] = torch.empty((n, ho, wo, num_classes), dtype=torch.float32, device=dev)
    if want_label and 'label' not in out:
        out['label'] = torch.empty((n, ho, wo), dtype=torch.int64, device=dev)
    if scale is not None:
        _need(scale, torch.float32, 'scale')
        _need(shift, torch.float32, 'shift')
        rc = _lib.lib().xv_decoder_head_affine_fwd(fused.xv(), _ptr(scale), _ptr(shift), _ptr(w_score), _ptr(b_score),
                                                  num_classes, _ptr(out.get('score') if want_score else None),
                                                  _ptr(out.get('prob') if want_prob else None),
                                                  _ptr(out.get('label') if want_label else None), _stream())
        _lib.check(rc, 'xv_decoder_head_affine_fwd')
        return out
    ws = workspace if workspace is not None else _head_workspace(fused, num_classes)
    rc = _lib.lib().xv_decoder_head_fwd(fused.xv(), _ptr(w_score), _ptr(b_score), num_classes,
                                       _ptr(out.get('score') if want_score else None),
                                       _ptr(out.get('prob') if want_prob else None),
                                       _ptr(out.get('label') if want_label else None), _ptr(ws), ws.numel() * 4,
                                       _stream())
    _lib.check(rc, 'xv_decoder_head_fwd')
    return out


def score_lowres(fused, w_score, num_classes, S):
    """S[n][i][j][k] = fused . Ws at 1/8 resolution (float32 [N][h+2][w+2][CP], CP = C rounded up to 4)."""
    _lib.check(_lib.lib().xv_score_lowres(fused.xv(), _ptr(w_score), int(num_classes), _ptr(S), _stream()), 'xv_score_lowres')
    return S


def decoder_head_from_scores(S, b_score, n, hi, wi, num_classes, score=None, prob=None, label=None):
    """The second half of decoder_head_fwd on low-resolution scores S (float32 [n][hi+2][wi+2][CP], zero border, e.g. from
    score_lowres): the x8 interpolation + bias -> whichever of score / prob (float32 [n, 8hi, 8wi, C]) and label (int64
    [n, 8hi, 8wi]) are given, written in place.  The label alone into a 16-byte aligned buffer runs four pixels per thread."""
    _need(S, torch.float32, 'S')
    _need(b_score, torch.float32, 'b_score')
    rc = _lib.lib().xv_decoder_head_from_scores(_ptr(S), _ptr(b_score), int(n), int(hi), int(wi), int(num_classes), _ptr(score),
                                               _ptr(prob), _ptr(label), _stream())
    _lib.check(rc, 'xv_decoder_head_from_scores')
    return score, prob, label


def fused_head(Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, tab, logprior, lognorm=None, out=None):
    """Both experts' low-resolution scores -> the fused label map (int64 [n, 8hi, 8wi]); lognorm given = Dirichlet
    fusion (tab = alpha - 1), else Bayes (tab = log-likelihood tables)."""
    if out is None:
        out = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=Sa.device)
    rc = _lib.lib().xv_fused_head_fwd(_ptr(Sa), _ptr(Sb), _ptr(bias_a), _ptr(bias_b), n, hi, wi, int(num_classes),
                                     0 if lognorm is None else 1, _ptr(tab), _ptr(lognorm), _ptr(logprior), _ptr(out),
                                     _stream())
    _lib.check(rc, 'xv_fused_head_fwd')
    return out


def _check_lowres_pair(Sa, Sb, n, hi, wi, num_classes, labels):
    cp = (int(num_classes) + 3) // 4 * 4
    for name, S in (('Sa', Sa), ('Sb', Sb)):
        _need(S, torch.float32, name)
        if tuple(S.shape) != (n, hi + 2, wi + 2, cp):
            raise ValueError('low-resolution scores %s of shape %s, expected %s' % (name, tuple(S.shape), (n, hi + 2, wi + 2, cp)))
    _check_labels(labels, n, hi, wi)


def _check_labels(labels, n, hi, wi):
    """The ground truth of a counting head: int32, one label per output pixel."""
    _need(labels, torch.int32, 'labels')
    if labels.numel() != n * hi * wi * 64:
        raise ValueError('labels of shape %s, expected %s' % (tuple(labels.shape), (n, 8 * hi, 8 * wi)))


def _label_output(out, n, hi, wi, device):
    """The label map a head writes, int64 [n, 8hi, 8wi]: made here when None, else checked."""
    if out is None:
        return torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=device)
    if out.dtype != torch.int64 or out.numel() != n * hi * wi * 64:
        raise ValueError('out must be int64 of %d elements' % (n * hi * wi * 64))
    return out


# ---- what the heads over two to four experts' low-resolution scores check before they launch (fused_head_multi and its six
# siblings).  Which layer refuses what differs between the siblings ON PURPOSE and is pinned by
# tests/test_multi_expert_python_refusals_gpu.py: fused_head_multi leaves the expert count, the mode and missing tables to the
# native check (XvError, XV_EINVAL); the counting form leaves the expert count to its capacity query; the others refuse here.

def _check_experts(scores, biases, n, hi, wi, num_classes, what=None):
    """(scores, biases, E, C): lists of equal length, every score a float32 CUDA tensor [n, hi+2, wi+2, CP], every bias of C
    values.  `what` names a head that refuses anything but two to four experts here; None leaves the count to the caller."""
    scores, biases = list(scores), list(biases)
    if len(scores) != len(biases):
        raise ValueError('%d score tensors but %d biases' % (len(scores), len(biases)))
    E, C = len(scores), int(num_classes)
    if what is not None and not 2 <= E <= 4:
        raise ValueError('%s takes two to four experts, got %d' % (what, E))
    cp = (C + 3) // 4 * 4
    for i, (S, b) in enumerate(zip(scores, biases)):
        _need(S, torch.float32, 'scores[%d]' % i)
        _need(b, torch.float32, 'biases[%d]' % i)
        if tuple(S.shape) != (n, hi + 2, wi + 2, cp):
            raise ValueError('low-resolution scores %d of shape %s, expected %s' % (i, tuple(S.shape), (n, hi + 2, wi + 2, cp)))
        if b.numel() != C:
            raise ValueError('bias %d of %d values, expected %d' % (i, b.numel(), C))
    return scores, biases, E, C


def _check_fusion_tables(mode, E, C, tab, lognorm, logprior, required=True, per_point=False):
    """The fusion tables of a multi-expert head for `mode`: Bayes tab [E,C,C] and logprior [C]; Dirichlet tab [E,C,C], lognorm
    [E,C] and logprior [C]; the mean none.  required=False (fused_head_multi) checks the tables that are given and leaves the
    mode and what is missing to the native check.  per_point (the counting form) takes G parameter sets -- logprior [G,C],
    the Dirichlet tab [G,E,C,C] and lognorm [G,E,C], the Bayes tab shared -- and G is returned (1 otherwise)."""
    if required:
        if mode == 2:
            if tab is not None or lognorm is not None or logprior is not None:
                raise ValueError('the mean takes no tables')
            return 1
        if tab is None or logprior is None or (mode == 1 and lognorm is None):
            raise ValueError('mode %d needs tab and logprior%s' % (mode, ', lognorm' if mode == 1 else ''))
        if mode == 0 and lognorm is not None:
            raise ValueError('Bayes fusion takes no lognorm')
    G, lead = 1, ()
    if per_point:
        G = int(logprior.shape[0]) if logprior.dim() == 2 else 0
        lead = (G,)
    for name, t, shape in (('tab', tab, (lead if mode == 1 else ()) + (E, C, C)), ('lognorm', lognorm, lead + (E, C)),
                           ('logprior', logprior, lead + (C,))):
        if t is not None:
            _need(t, torch.float32, name)
            if G < 1 or tuple(t.shape) != shape:
                raise ValueError('%s of shape %s, expected %s%s' % (name, tuple(t.shape), shape,
                                                                    ' with G >= 1' if per_point else ''))
    return G


def fused_head_grid_capacity(num_classes):
    """Most grid points one xv_fused_head_grid_score_fwd launch takes at this class count."""
    return int(_lib.lib().xv_fused_head_grid_capacity(int(num_classes)))


def fused_head_grid_score(Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, tab, lognorm, logprior, labels, cm=None,
                          max_workgroups=0):
    """Both experts' low-resolution scores, fused under G Dirichlet parameter sets at once (tab float32 [G,2,C,C] = alpha - 1,
    lognorm [G,2,C], logprior [G,C], each set as fused_head takes one) and counted against labels (int32 [n, 8hi, 8wi]):
    accumulates into cm (int64 [G,C,C], rows = ground truth; made here when None) and returns it.  More sets than one launch
    holds (fused_head_grid_capacity) go in several launches on the same scores."""
    C = int(num_classes)
    _check_lowres_pair(Sa, Sb, n, hi, wi, C, labels)
    for name, t in (('bias_a', bias_a), ('bias_b', bias_b), ('tab', tab), ('lognorm', lognorm), ('logprior', logprior)):
        _need(t, torch.float32, name)
    G = tab.shape[0]
    if G < 1 or tuple(tab.shape) != (G, 2, C, C) or tuple(lognorm.shape) != (G, 2, C) or tuple(logprior.shape) != (G, C):
        raise ValueError('tables of shapes %s, %s, %s, expected [G,2,C,C], [G,2,C], [G,C] with C = %d' % (
            tuple(tab.shape), tuple(lognorm.shape), tuple(logprior.shape), C))
    if cm is None:
        cm = torch.zeros((G, C, C), dtype=torch.int64, device=Sa.device)
    _need(cm, torch.int64, 'cm')
    if tuple(cm.shape) != (G, C, C):
        raise ValueError('cm of shape %s, expected %s' % (tuple(cm.shape), (G, C, C)))
    cap = fused_head_grid_capacity(C)
    if cap < 1:
        raise ValueError('no grid-scoring head for %d classes' % C)
    for g0 in range(0, G, cap):
        g1 = min(G, g0 + cap)
        rc = _lib.lib().xv_fused_head_grid_score_fwd(_ptr(Sa), _ptr(Sb), _ptr(bias_a), _ptr(bias_b), n, hi, wi, C, g1 - g0,
                                                    _ptr(tab[g0:g1]), _ptr(lognorm[g0:g1]), _ptr(logprior[g0:g1]), _ptr(labels),
                                                    _ptr(cm[g0:g1]), int(max_workgroups), _stream())
        _lib.check(rc, 'xv_fused_head_grid_score_fwd')
    return cm


def fused_head_joint_hist(Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, labels, hist=None, max_workgroups=0):
    """Both experts' low-resolution scores -> the joint histogram of (ground truth, label of expert a, label of expert b):
    accumulates into hist (int64 [C,C,C]; made here when None) over the pixels with a valid label and returns it.  At most 20
    classes."""
    C = int(num_classes)
    _check_lowres_pair(Sa, Sb, n, hi, wi, C, labels)
    _need(bias_a, torch.float32, 'bias_a')
    _need(bias_b, torch.float32, 'bias_b')
    if labels.data_ptr() & 15:            # (a slice of a larger map: the kernel reads label quads with 16-byte loads)
        labels = labels.clone()
    if hist is None:
        hist = torch.zeros((C, C, C), dtype=torch.int64, device=Sa.device)
    _need(hist, torch.int64, 'hist')
    if tuple(hist.shape) != (C, C, C):
        raise ValueError('hist of shape %s, expected %s' % (tuple(hist.shape), (C, C, C)))
    rc = _lib.lib().xv_fused_head_joint_hist_fwd(_ptr(Sa), _ptr(Sb), _ptr(bias_a), _ptr(bias_b), n, hi, wi, C, _ptr(labels),
                                                _ptr(hist), int(max_workgroups), _stream())
    _lib.check(rc, 'xv_fused_head_joint_hist_fwd')
    return hist


def upload_group_ids(groups, num_groups, device):
    """One group id per image (a host sequence, numpy array or CPU tensor), checked HERE -- integers, every one in
    [0, num_groups) -- and uploaded as the int32 tensor the grouped kernels index with.  A pass over many batches calls this
    once for all its images and hands the grouped ops slices of the result."""
    G = int(num_groups)
    if G < 1:
        raise ValueError('num_groups must be at least 1, got %d' % G)
    ids = np.asarray(groups.cpu() if isinstance(groups, torch.Tensor) else groups)
    if ids.ndim != 1 or ids.dtype.kind not in 'iu':
        raise ValueError('groups must be integers, one per image, got shape %s of dtype %s' % (ids.shape, ids.dtype))
    if ids.size and (ids.min() < 0 or ids.max() >= G):
        raise ValueError('group ids must lie in [0, %d), got %d .. %d' % (G, ids.min(), ids.max()))
    return torch.from_numpy(ids.astype(np.int32)).to(device)


def _group_ids(groups, n, num_groups, device):
    """The int32 [n] device tensor of a grouped launch: `groups` from the host goes through upload_group_ids; a CUDA int32
    tensor is taken as (a slice of) what upload_group_ids returned -- checked there, only its length is checked here."""
    if isinstance(groups, torch.Tensor) and groups.is_cuda:
        _need(groups, torch.int32, 'groups')
        if int(num_groups) < 1 or tuple(groups.shape) != (n,):
            raise ValueError('groups of shape %s for %d images and %d groups' % (tuple(groups.shape), n, int(num_groups)))
        return groups
    ids = upload_group_ids(groups, num_groups, device)
    if ids.numel() != n:
        raise ValueError('groups must be %d integers (one per image), got %d' % (n, ids.numel()))
    return ids


def fused_head_joint_hist_grouped(Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, labels, groups, num_groups, hist=None,
                                  max_workgroups=0):
    """fused_head_joint_hist per group of images: `groups` holds one id in [0, num_groups) per image (host side: checked here
    before anything is launched; or a device slice of upload_group_ids' result); accumulates into hist (int64 [G,C,C,C]; made here, zeroed, when None) and returns it."""
    C, G = int(num_classes), int(num_groups)
    _check_lowres_pair(Sa, Sb, n, hi, wi, C, labels)
    _need(bias_a, torch.float32, 'bias_a')
    _need(bias_b, torch.float32, 'bias_b')
    ids = _group_ids(groups, n, G, Sa.device)
    if labels.data_ptr() & 15:            # (a slice of a larger map: the kernel reads label quads with 16-byte loads)
        labels = labels.clone()
    if hist is None:
        hist = torch.zeros((G, C, C, C), dtype=torch.int64, device=Sa.device)
    _need(hist, torch.int64, 'hist')
    if tuple(hist.shape) != (G, C, C, C):
        raise ValueError('hist of shape %s, expected %s' % (tuple(hist.shape), (G, C, C, C)))
    rc = _lib.lib().xv_fused_head_joint_hist_grouped_fwd(_ptr(Sa), _ptr(Sb), _ptr(bias_a), _ptr(bias_b), n, hi, wi, C,
                                                        _ptr(labels), _ptr(ids), G, _ptr(hist), int(max_workgroups), _stream())
    _lib.check(rc, 'xv_fused_head_joint_hist_grouped_fwd')
    return hist


def fused_head_average(Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, out=None):
    """Both experts' low-resolution scores -> the average-fused label map (int64 [n, 8hi, 8wi]): the labels of average_fuse on
    the two probability maps decoder_head_from_scores writes, without those maps."""
    if out is None:
        out = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=Sa.device)
    rc = _lib.lib().xv_fused_head_average_fwd(_ptr(Sa), _ptr(Sb), _ptr(bias_a), _ptr(bias_b), n, hi, wi, int(num_classes),
                                             _ptr(out), _stream())
    _lib.check(rc, 'xv_fused_head_average_fwd')
    return out


FUSED_HEAD_MODES = {'bayes': 0, 'dirichlet': 1, 'mean': 2}


def fused_head_multi(scores, biases, n, hi, wi, num_classes, mode, tab=None, lognorm=None, logprior=None, out=None):
    """Two to four experts' low-resolution scores (lists of E tensors, scores float32 [n][hi+2][wi+2][CP], biases float32 [C])
    -> the fused label map (int64 [n, 8hi, 8wi]) in one launch.  mode 0 / 'bayes': tab = log-likelihood tables [E,C,C] and
    logprior [C], the labels of bayes_fuse on the experts' label maps; 1 / 'dirichlet': tab = alpha - 1 [E,C,C], lognorm [E,C],
    logprior, the labels of dirichlet_fuse on their probability maps; 2 / 'mean': no tables, the labels of average_fuse --
    bit for bit, and none of those maps is written."""
    mode = FUSED_HEAD_MODES.get(mode, mode)
    scores, biases, E, C = _check_experts(scores, biases, n, hi, wi, num_classes)
    _check_fusion_tables(mode, E, C, tab, lognorm, logprior, required=False)
    out = _label_output(out, n, hi, wi, scores[0].device)
    rc = _lib.lib().xv_fused_head_multi_fwd(_ptr_array(scores), _ptr_array(biases), E, int(n), int(hi), int(wi), C, int(mode),
                                           _ptr(tab), _ptr(lognorm), _ptr(logprior), _ptr(out), _stream())
    _lib.check(rc, 'xv_fused_head_multi_fwd')
    return out


def fused_head_multi_count_capacity(num_classes, num_experts, mode):
    """Most parameter sets one xv_fused_head_multi_count_fwd launch takes (0: nothing of that kind is served)."""
    mode = FUSED_HEAD_MODES.get(mode, mode)
    return int(_lib.lib().xv_fused_head_multi_count_capacity(int(num_classes), int(num_experts), int(mode)))


def fused_head_multi_count(scores, biases, n, hi, wi, num_classes, mode, labels, tab=None, lognorm=None, logprior=None,
                           groups=None, num_groups=1, cm=None, expert_cm=None, max_workgroups=0):
    """Counting form of fused_head_multi: two to four experts' low-resolution scores, fused under G parameter sets at once and
    counted against labels (int32 [n, 8hi, 8wi]) without a label map.  mode 0 / 'bayes': tab [E,C,C] shared by all sets,
    logprior [G,C]; 1 / 'dirichlet': tab [G,E,C,C], lognorm [G,E,C], logprior [G,C]; 2 / 'mean': no tables, G = 1.
    Accumulates into cm (int64 [num_groups,G,C,C], or [G,C,C] without groups; rows = ground truth; made here when None) and
    returns it.  expert_cm (int64 [num_groups,E,C,C] / [E,C,C]) also takes every expert's own confusion matrix.  `groups`
    as fused_head_joint_hist_grouped takes it.  More sets than one launch holds (fused_head_multi_count_capacity) go in
    several launches on the same scores; expert_cm is counted by the first one only."""
    mode = FUSED_HEAD_MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError('unknown fused head mode %r' % (mode,))
    scores, biases, E, C = _check_experts(scores, biases, n, hi, wi, num_classes)
    _check_labels(labels, n, hi, wi)
    # (a lognorm handed to the Bayes form is ignored, as it always was)
    G = _check_fusion_tables(mode, E, C, tab, lognorm if mode != 0 else None, logprior, per_point=True)
    NG = int(num_groups)
    cm, ids = _grouped_output(cm, 'cm', groups, n, NG, (G, C, C), scores[0].device)
    lead = (NG,) if groups is not None else ()
    if expert_cm is not None:
        _need(expert_cm, torch.int64, 'expert_cm')
        if tuple(expert_cm.shape) != lead + (E, C, C):
            raise ValueError('expert_cm of shape %s, expected %s' % (tuple(expert_cm.shape), lead + (E, C, C)))
    cap = fused_head_multi_count_capacity(C, E, mode)
    if cap < 1:
        raise ValueError('no counting head for %d experts, %d classes, mode %d' % (E, C, mode))
    S_arr, b_arr = _ptr_array(scores), _ptr_array(biases)
    for g0 in range(0, G, cap):
        g1 = min(G, g0 + cap)
        # a launch writes cm [num_groups][g1 - g0][C][C] densely: a slice of the points of a grouped cm is counted apart
        part = cm if (g0, g1) == (0, G) else (cm[g0:g1] if groups is None else
                                             torch.zeros((NG, g1 - g0, C, C), dtype=torch.int64, device=cm.device))
        rc = _lib.lib().xv_fused_head_multi_count_fwd(
            S_arr, b_arr, E, int(n), int(hi), int(wi), C, int(mode), g1 - g0, _ptr(tab if mode != 1 else tab[g0:g1]),
            _ptr(None if mode != 1 else lognorm[g0:g1]), _ptr(None if mode == 2 else logprior[g0:g1]), _ptr(labels), _ptr(ids),
            NG, _ptr(part), _ptr(expert_cm if g0 == 0 else None), int(max_workgroups), _stream())
        _lib.check(rc, 'xv_fused_head_multi_count_fwd')
        if part is not cm and groups is not None:
            cm[:, g0:g1] += part
    return cm


def fused_head_multi_agreement(scores, biases, n, hi, wi, num_classes, mode, labels, tab=None, lognorm=None, logprior=None,
                               groups=None, num_groups=1, table=None, max_workgroups=0):
    """Two to four experts' low-resolution scores (as fused_head_multi takes them, with its tables for `mode`) -> the
    expert-agreement table against labels (int32 [n, 8hi, 8wi]) in one launch, without a label map:
    table[label][mask][unanimous][outcome] += 1 over the pixels with 0 <= label < C, where bit e of mask says that expert e's
    label is right, unanimous that all experts give one label, and outcome is 0 (the fused label is right), 1 (wrong, but some
    expert's label) or 2 (wrong and no expert's label).  Accumulates into table (int64 [num_groups, C, 2^E, 2, 3], or
    [C, 2^E, 2, 3] without groups; made here, zeroed, when None) and returns it.  `groups` as fused_head_joint_hist_grouped
    takes it."""
    mode = FUSED_HEAD_MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError('unknown fused head mode %r' % (mode,))
    scores, biases, E, C = _check_experts(scores, biases, n, hi, wi, num_classes, 'the agreement head')
    _check_labels(labels, n, hi, wi)
    _check_fusion_tables(mode, E, C, tab, lognorm, logprior)
    table, ids = _grouped_output(table, 'table', groups, n, num_groups, (C, 1 << E, 2, 3), scores[0].device)
    rc = _lib.lib().xv_fused_head_multi_agreement_fwd(
        _ptr_array(scores), _ptr_array(biases), E, int(n), int(hi), int(wi), C, int(mode), _ptr(tab), _ptr(lognorm),
        _ptr(logprior), _ptr(labels), _ptr(ids), int(num_groups), _ptr(table), int(max_workgroups), _stream())
    _lib.check(rc, 'xv_fused_head_multi_agreement_fwd')
    return table


def agreement_table(labels, expert_labels, fused, num_classes, groups=None, num_groups=1, table=None):
    """The table of fused_head_multi_agreement from MATERIALISED maps: labels int32 [n, ...], expert_labels a list of two to four
    int64 maps of that shape (one per expert, in the order of the mask's bits), fused int64 of that shape.  The image axis comes
    first (it is what `groups` indexes).  Accumulates into table (made here, zeroed, when None) and returns it."""
    expert_labels = list(expert_labels)
    E, C = len(expert_labels), int(num_classes)
    if not 2 <= E <= 4:
        raise ValueError('the agreement table takes two to four experts, got %d' % E)
    _need(labels, torch.int32, 'labels')
    _need(fused, torch.int64, 'fused')
    if labels.dim() < 2 or labels.numel() == 0:
        raise ValueError('labels of shape %s, expected non-empty [n, ...]' % (tuple(labels.shape),))
    for i, lab in enumerate(expert_labels):
        _need(lab, torch.int64, 'expert_labels[%d]' % i)
    for name, t in [('fused', fused)] + [('expert_labels[%d]' % i, lab) for i, lab in enumerate(expert_labels)]:
        if t.shape != labels.shape:
            raise ValueError('%s of shape %s, labels of shape %s' % (name, tuple(t.shape), tuple(labels.shape)))
    n = labels.shape[0]
    table, ids = _grouped_output(table, 'table', groups, n, num_groups, (C, 1 << E, 2, 3), labels.device)
    rc = _lib.lib().xv_agreement_table(_ptr(labels), _ptr_array(expert_labels), E, _ptr(fused), _ptr(ids), n,
                                       labels.numel() // n, C, int(num_groups), _ptr(table), _stream())
    _lib.check(rc, 'xv_agreement_table')
    return table


# ---- calibration scoring (csrc/calibration.hip): reliability tables int64 [T, NB, 3] = (count, correct, sum of the confidence in
# 2^-24 steps) per temperature and confidence bin, and the NLL sums float64 [T]; calibration.calibration_measures reads them

def calibration_capacity(bin_bits, num_tables=1):
    """Temperatures one calibration launch serves with `num_tables` tables per temperature (1: the fusion alone, 1 + E: the
    experts' beside it); 0 outside the supported ranges.  No GPU call."""
    return int(_lib.lib().xv_calibration_capacity(int(bin_bits), int(num_tables)))


def _calibration_temperatures(temperatures, bin_bits):
    """The temperatures as a list of floats and the bin count, checked here as the kernels check them."""
    temps = [float(t) for t in np.atleast_1d(np.asarray(temperatures, np.float64))]
    if not temps or not all(np.isfinite(t) and np.float32(t) > 0 and np.isfinite(np.float32(t)) for t in temps):
        raise ValueError('temperatures must be finite and positive, at least one, got %r' % (temperatures,))
    if not 4 <= int(bin_bits) <= 10:
        raise ValueError('bin_bits must lie in 4..10, got %r' % (bin_bits,))
    return temps, 1 << int(bin_bits)


def _calibration_outputs(table, nll, name, groups, n, num_groups, lead, NT, NB, device):
    """(table, nll, group ids): int64 [num_groups, *lead, NT, NB, 3] and float64 [num_groups, *lead, NT] (without the group axis
    when there are no groups), zeroed ones made here when none are given."""
    table, ids = _grouped_output(table, name, groups, n, num_groups, tuple(lead) + (NT, NB, 3), device)
    shape = tuple(table.shape[:-2])
    if nll is None:
        nll = torch.zeros(shape, dtype=torch.float64, device=device)
    _need(nll, torch.float64, name.replace('table', 'nll'))
    if tuple(nll.shape) != shape:
        raise ValueError('%s of shape %s, expected %s' % (name.replace('table', 'nll'), tuple(nll.shape), shape))
    return table, nll, ids


def _calibration_chunks(temps, cap, grouped, outs):
    """Temperature chunks of at most `cap`: (c_float array, t0, t1, [(launch target, its final tensor or None)]).  A launch
    writes its temperatures densely: without groups a slice of the temperature axis (the leading one of a table, the one behind
    the experts of an expert table, which is then counted apart) is handed over; otherwise a zeroed stand-in that the caller
    adds afterwards."""
    NT = len(temps)
    for t0 in range(0, NT, cap):
        t1 = min(NT, t0 + cap)
        targets = []
        for out, taxis in outs:
            if out is None:
                targets.append((None, None))
            elif (t0, t1) == (0, NT):
                targets.append((out, None))
            elif not grouped and taxis == 0:
                targets.append((out[t0:t1], None))
            else:
                shape = list(out.shape)
                shape[taxis + (1 if grouped else 0)] = t1 - t0
                targets.append((torch.zeros(shape, dtype=out.dtype, device=out.device), out))
        yield (ctypes.c_float * (t1 - t0))(*temps[t0:t1]), t0, t1, targets


def _calibration_merge(targets, t0, t1, grouped, taxes):
    for (part, out), taxis in zip(targets, taxes):
        if out is not None:
            axis = taxis + (1 if grouped else 0)
            out.narrow(axis, t0, t1 - t0).add_(part)


def calibration_table(values, labels, temperatures=1.0, bin_bits=10, kind=0, num_classes=None, groups=None, num_groups=1,
                      table=None, nll=None):
    """The reliability table of a MATERIALISED map: values float32 [n, ..., C], class scores in the log domain (kind 0) or
    probabilities (kind 1: ln(1e-20 + p) after the winner is taken); labels int32 [n, ...].  Per temperature T and pixel with
    0 <= label < C: conf = 1 / sum_k exp((s[k] - s[win]) / T), q = int(conf 2^24), bin = min(q >> (24 - bin_bits), NB - 1);
    table[t][bin] += (1, win == label, q) and nll[t] += min(ln z - (s[label] - s[win]) / T, -ln 1e-10).  Accumulates into
    table (int64 [T, NB, 3], [num_groups, T, NB, 3] with groups) and nll (float64 [T] / [num_groups, T]), made here, zeroed,
    when None, and returns (table, nll).  More temperatures than one launch holds (calibration_capacity) go in several
    launches.  `groups` as fused_head_joint_hist_grouped takes it; the image axis comes first."""
    temps, NB = _calibration_temperatures(temperatures, bin_bits)
    if kind not in (0, 1):
        raise ValueError('kind must be 0 (scores) or 1 (probabilities), got %r' % (kind,))
    _need(values, torch.float32, 'values')
    _need(labels, torch.int32, 'labels')
    C = int(values.shape[-1]) if num_classes is None else int(num_classes)
    if not 2 <= C <= 32:
        raise ValueError('the calibration table takes 2..32 classes, got %d' % C)
    if labels.dim() < 2 or labels.numel() == 0 or tuple(values.shape) != tuple(labels.shape) + (C,):
        raise ValueError('values of shape %s, labels of shape %s, %d classes: expected [n, ..., C] and non-empty [n, ...]'
                         % (tuple(values.shape), tuple(labels.shape), C))
    n = labels.shape[0]
    table, nll, ids = _calibration_outputs(table, nll, 'table', groups, n, num_groups, (), len(temps), NB, values.device)
    cap = calibration_capacity(bin_bits, 1)
    for arr, t0, t1, targets in _calibration_chunks(temps, cap, groups is not None, [(table, 0), (nll, 0)]):
        rc = _lib.lib().xv_calibration_table(_ptr(values), int(kind), _ptr(labels), _ptr(ids), n, labels.numel() // n, C,
                                             ctypes.cast(arr, ctypes.c_void_p), t1 - t0, int(bin_bits), int(num_groups),
                                             _ptr(targets[0][0]), _ptr(targets[1][0]), _stream())
        _lib.check(rc, 'xv_calibration_table')
        _calibration_merge(targets, t0, t1, groups is not None, (0, 0))
    return table, nll


def fused_head_multi_calibration(scores, biases, n, hi, wi, num_classes, mode, labels, temperatures=1.0, bin_bits=10, tab=None,
                                 lognorm=None, logprior=None, groups=None, num_groups=1, table=None, nll=None, experts=False,
                                 expert_table=None, expert_nll=None, max_workgroups=0):
    """Two to four experts' low-resolution scores (as fused_head_multi takes them, with its tables for `mode`) -> the
    reliability table of the FUSED posterior against labels (int32 [n, 8hi, 8wi]) in one launch, as calibration_table counts the
    fused score map (Bayes, Dirichlet) or the mean probabilities (kind 1), without that map.  Returns (table, nll); with
    experts=True (or expert_table / expert_nll given) also every expert's own table from its logits: (table, nll, expert_table
    int64 [E, T, NB, 3], expert_nll float64 [E, T]), each with a leading group axis under `groups`.  All are accumulated into;
    zeroed ones are made here when None.  More temperatures than one launch holds go in several launches on the same scores."""
    mode = FUSED_HEAD_MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError('unknown fused head mode %r' % (mode,))
    temps, NB = _calibration_temperatures(temperatures, bin_bits)
    scores, biases, E, C = _check_experts(scores, biases, n, hi, wi, num_classes, 'the calibration head')
    _check_labels(labels, n, hi, wi)
    _check_fusion_tables(mode, E, C, tab, lognorm, logprior)
    device, NT, grouped = scores[0].device, len(temps), groups is not None
    table, nll, ids = _calibration_outputs(table, nll, 'table', groups, n, num_groups, (), NT, NB, device)
    experts = bool(experts) or expert_table is not None or expert_nll is not None
    if experts:
        expert_table, expert_nll, _ = _calibration_outputs(expert_table, expert_nll, 'expert_table', ids, n, num_groups, (E,),
                                                           NT, NB, device)
    cap = calibration_capacity(bin_bits, 1 + E if experts else 1)
    if cap < 1:
        raise ValueError('no calibration head for %d bin bits and %d experts' % (bin_bits, E))
    S_arr, b_arr = _ptr_array(scores), _ptr_array(biases)
    outs = [(table, 0), (nll, 0), (expert_table, 1), (expert_nll, 1)]
    for arr, t0, t1, targets in _calibration_chunks(temps, cap, grouped, outs):
        rc = _lib.lib().xv_fused_head_multi_calibration_fwd(
            S_arr, b_arr, E, int(n), int(hi), int(wi), C, int(mode), _ptr(tab), _ptr(lognorm), _ptr(logprior), _ptr(labels),
            _ptr(ids), int(num_groups), ctypes.cast(arr, ctypes.c_void_p), t1 - t0, int(bin_bits), _ptr(targets[0][0]),
            _ptr(targets[1][0]), _ptr(targets[2][0]), _ptr(targets[3][0]), int(max_workgroups), _stream())
        _lib.check(rc, 'xv_fused_head_multi_calibration_fwd')
        _calibration_merge(targets, t0, t1, grouped, (0, 0, 1, 1))
    return (table, nll, expert_table, expert_nll) if experts else (table, nll)


# ---- confidence maps (csrc/confidence.hip): the confidence the tables above count, written per pixel at one temperature

CONFIDENCE_MAPS = {'label': torch.int64, 'confidence': torch.float32, 'entropy': torch.float32, 'margin': torch.float32}


def _confidence_outputs(want, out, shape, device, temperature, threshold):
    """{key: tensor} of the maps in `want` (from label, confidence, entropy, margin; at least one), taken from `out` where it
    holds them, made here otherwise, and the temperature and threshold checked as the kernels check them."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or len(set(want)) != len(want) or any(k not in CONFIDENCE_MAPS for k in want):
        raise ValueError('want names one or more of %s, each once, got %r' % (', '.join(CONFIDENCE_MAPS), want))
    T, thr = float(temperature), float(threshold)
    if not (np.isfinite(T) and np.float32(T) > 0 and np.isfinite(np.float32(T))):
        raise ValueError('the temperature must be finite and positive, got %r' % (temperature,))
    if not 0.0 <= thr <= 1.0:
        raise ValueError('the threshold must lie in [0, 1], got %r' % (threshold,))
    maps = {}
    for k in want:
        t = None if out is None else out.get(k)
        if t is None:
            t = torch.empty(shape, dtype=CONFIDENCE_MAPS[k], device=device)
        _need(t, CONFIDENCE_MAPS[k], 'out[%r]' % k)
        if t.numel() != int(np.prod(shape)):
            raise ValueError('out[%r] of shape %s, expected %s' % (k, tuple(t.shape), tuple(shape)))
        maps[k] = t
    return maps, T, thr


def confidence_map(values, temperature=1.0, kind=0, want=('label', 'confidence'), threshold=0.0, void_label=-1, out=None):
    """A MATERIALISED map -- values float32 [n, ..., C], class scores in the log domain (kind 0) or probabilities (kind 1:
    ln(1e-20 + p) after the winner is taken) -- to {key: device tensor [n, ...]} for the keys of `want`: 'label' int64, the
    first maximum, or void_label where the confidence is below `threshold`; 'confidence' = 1 / sum_k exp((s[k] - s[win]) / T),
    whose int(conf 2^24) is the q calibration_table counts; 'entropy' of that softmax in nats; 'margin', the confidence minus
    the second largest probability.  `out` may hold tensors to write into."""
    if kind not in (0, 1):
        raise ValueError('kind must be 0 (scores) or 1 (probabilities), got %r' % (kind,))
    _need(values, torch.float32, 'values')
    if values.dim() < 2 or values.numel() == 0 or not 2 <= int(values.shape[-1]) <= 32:
        raise ValueError('values of shape %s, expected non-empty [n, ..., C] with 2..32 classes' % (tuple(values.shape),))
    shape, C = tuple(values.shape[:-1]), int(values.shape[-1])
    maps, T, thr = _confidence_outputs(want, out, shape, values.device, temperature, threshold)
    n = shape[0]
    rc = _lib.lib().xv_confidence_map(_ptr(values), int(kind), n, values.numel() // (n * C), C, T, thr, int(void_label),
                                      _ptr(maps.get('label')), _ptr(maps.get('confidence')), _ptr(maps.get('entropy')),
                                      _ptr(maps.get('margin')), _stream())
    _lib.check(rc, 'xv_confidence_map')
    return maps


def fused_head_multi_confidence(scores, biases, n, hi, wi, num_classes, mode, temperature=1.0, tab=None, lognorm=None,
                                logprior=None, want=('label', 'confidence'), threshold=0.0, void_label=-1, out=None):
    """Two to four experts' low-resolution scores (as fused_head_multi takes them, with its tables for `mode`) -> the maps of
    confidence_map for the FUSED posterior, [n, 8hi, 8wi] each, in one launch: what confidence_map gives on the fused score
    map (Bayes, Dirichlet) or the mean probabilities (kind 1), without that map.  With threshold 0 'label' is the label of
    fused_head_multi, bit for bit."""
    mode = FUSED_HEAD_MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError('unknown fused head mode %r' % (mode,))
    scores, biases, E, C = _check_experts(scores, biases, n, hi, wi, num_classes, 'the confidence head')
    _check_fusion_tables(mode, E, C, tab, lognorm, logprior)
    maps, T, thr = _confidence_outputs(want, out, (n, 8 * hi, 8 * wi), scores[0].device, temperature, threshold)
    rc = _lib.lib().xv_fused_head_multi_confidence_fwd(
        _ptr_array(scores), _ptr_array(biases), E, int(n), int(hi), int(wi), C, int(mode), _ptr(tab), _ptr(lognorm),
        _ptr(logprior), T, thr, int(void_label), _ptr(maps.get('label')), _ptr(maps.get('confidence')),
        _ptr(maps.get('entropy')), _ptr(maps.get('margin')), _stream())
    _lib.check(rc, 'xv_fused_head_multi_confidence_fwd')
    return maps


# ---- uncertainty benchmarks of a posterior (csrc/confidence_stats.hip): the confidence maps counted instead of written

CONFIDENCE_METRICS = ('entropy', 'least_confidence', 'small_margin')    # the order of the kernels' histograms


def _confidence_stats_tables(tables, C, device, mantissa_bits, octaves, labels, npix, lead=()):
    """The accumulators of one confidence_stats launch -- uncertainty_tables(C, device, 3, m, o), with `lead` (E,) in front of
    every shape for the experts' -- made here when None, else checked; labels int32 of npix values, or None."""
    if labels is not None:
        _need(labels, torch.int32, 'labels')
        if labels.numel() != npix:
            raise ValueError('labels of shape %s, expected %d values' % (tuple(labels.shape), npix))
    bins = int(octaves) << int(mantissa_bits)
    if tables is None:
        tables = uncertainty_tables(C, device, 3, mantissa_bits, octaves)
        if lead:
            tables = {k: t.new_zeros(tuple(lead) + tuple(t.shape)) for k, t in tables.items()}
    _need(tables['hist'], torch.int64, 'hist')
    _need(tables['nll'], torch.float64, 'nll')
    _need(tables['counts'], torch.int64, 'counts')
    shapes = {'hist': tuple(lead) + (3, 2, bins), 'nll': tuple(lead) + (C,), 'counts': tuple(lead) + (C,)}
    for k, shape in shapes.items():
        if tuple(tables[k].shape) != shape:
            raise ValueError('%s of shape %s, expected %s' % (k, tuple(tables[k].shape), shape))
    return tables


def confidence_stats(values, labels=None, temperature=1.0, kind=0, fixed_row=-1, mantissa_bits=5, octaves=24, tables=None):
    """The uncertainty benchmarks' statistic of a MATERIALISED map (xv_confidence_stats) -- values and kind as confidence_map
    takes them -- without writing a map: accumulates into `tables` (uncertainty_tables(C, device, 3, m, o), made here when
    None) hist[metric][row][bin] of the three CONFIDENCE_METRICS, larger = less certain, each one float32 operation from what
    confidence_map writes: 'entropy', 'least_confidence' = 1 - confidence, 'small_margin' = 1 - margin.  row = (label of the
    map != labels) over the pixels with a valid label, or `fixed_row` (0 / 1) for every pixel (labels may then be None); with
    labels also the NLL sums -- the nll_pixel of calibration_table at this temperature -- and class counts.  Values at or
    below 2^(1 - octaves) share bin 0: at the default 24 octaves that is the resolution limit of 1 - confidence in float32, so
    nothing a float32 confidence can tell apart is merged.  Returns the tables."""
    _need(values, torch.float32, 'values')
    if values.dim() < 2 or values.numel() == 0 or not 2 <= int(values.shape[-1]) <= 32:
        raise ValueError('values of shape %s, expected non-empty [n, ..., C] with 2..32 classes' % (tuple(values.shape),))
    n, C = int(values.shape[0]), int(values.shape[-1])
    npix = values.numel() // C
    tables = _confidence_stats_tables(tables, C, values.device, mantissa_bits, octaves, labels, npix)
    rc = _lib.lib().xv_confidence_stats(_ptr(values), int(kind), n, npix // n, C, float(temperature), _ptr(labels),
                                       int(mantissa_bits), int(octaves), int(fixed_row), _ptr(tables['hist']),
                                       _ptr(tables['nll']), _ptr(tables['counts']), _stream())
    _lib.check(rc, 'xv_confidence_stats')
    return tables


def fused_head_multi_confidence_stats(scores, biases, n, hi, wi, num_classes, mode, labels=None, temperature=1.0, tab=None,
                                      lognorm=None, logprior=None, fixed_row=-1, mantissa_bits=5, octaves=24, tables=None,
                                      experts=False, expert_tables=None):
    """Two to four experts' low-resolution scores (as fused_head_multi_confidence takes them, with its tables for `mode`) ->
    the tables of confidence_stats for the FUSED posterior in one launch: what confidence_stats counts on the fused score map
    (Bayes, Dirichlet) or the mean probabilities (kind 1), without that map.  experts=True (or expert_tables given: 'hist'
    [E, 3, 2, bins], 'nll' and 'counts' [E, C]) also counts every expert's own tables from its interpolated logits, its own
    label against `labels`.  Returns the tables, with experts (tables, expert_tables)."""
    mode = FUSED_HEAD_MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError('unknown fused head mode %r' % (mode,))
    scores, biases, E, C = _check_experts(scores, biases, n, hi, wi, num_classes, 'the confidence statistics head')
    _check_fusion_tables(mode, E, C, tab, lognorm, logprior)
    device, npix = scores[0].device, n * hi * wi * 64
    tables = _confidence_stats_tables(tables, C, device, mantissa_bits, octaves, labels, npix)
    experts = experts or expert_tables is not None
    if experts:
        expert_tables = _confidence_stats_tables(expert_tables, C, device, mantissa_bits, octaves, None, npix, lead=(E,))
    et = expert_tables if experts else {}
    rc = _lib.lib().xv_fused_head_multi_confidence_stats_fwd(
        _ptr_array(scores), _ptr_array(biases), E, int(n), int(hi), int(wi), C, int(mode), _ptr(tab), _ptr(lognorm),
        _ptr(logprior), float(temperature), _ptr(labels), int(mantissa_bits), int(octaves), int(fixed_row),
        _ptr(tables['hist']), _ptr(tables['nll']), _ptr(tables['counts']), _ptr(et.get('hist')), _ptr(et.get('nll')),
        _ptr(et.get('counts')), _stream())
    _lib.check(rc, 'xv_fused_head_multi_confidence_stats_fwd')
    return (tables, expert_tables) if experts else tables


# ---- label-tuple heads (csrc/tuple_lut.hip): the tuple of a pixel's expert labels is t = ((l_0 C + l_1) C + l_2) ..., expert
# 0 most significant: the row-major index of a [C]*E decision array

def tuple_capacity(num_classes, num_experts):
    """Do the three label-tuple heads serve this pair (C^E u32 counters within one workgroup's LDS)?  No GPU call."""
    return bool(_lib.lib().xv_tuple_capacity(int(num_classes), int(num_experts)))


def _check_tuple_experts(scores, biases, n, hi, wi, num_classes, what):
    """(scores, biases, E, C, T) of a label-tuple head, the shapes checked as fused_head_multi checks them."""
    scores, biases, E, C = _check_experts(scores, biases, n, hi, wi, num_classes, what)
    if not 2 <= C <= 32 or not tuple_capacity(C, E):
        raise ValueError('%s does not serve %d experts at %d classes (tuple_capacity)' % (what, E, C))
    return scores, biases, E, C, C ** E


def _check_tuple_lut(lut, T):
    _need(lut, torch.uint8, 'lut')
    if tuple(lut.shape) != (T,):
        raise ValueError('lut of shape %s, expected %s' % (tuple(lut.shape), (T,)))


def _grouped_output(out, name, groups, n, num_groups, cell_shape, device):
    """(out, group ids) of a grouped counting op: int64 [num_groups, *cell_shape], or cell_shape without groups; a zeroed one
    is made here when none is given."""
    NG = int(num_groups)
    ids = None
    if groups is not None:
        ids = _group_ids(groups, n, NG, device)
    elif NG != 1:
        raise ValueError('num_groups = %d without groups' % NG)
    shape = ((NG,) if groups is not None else ()) + tuple(cell_shape)
    if out is None:
        out = torch.zeros(shape, dtype=torch.int64, device=device)
    _need(out, torch.int64, name)
    if tuple(out.shape) != shape:
        raise ValueError('%s of shape %s, expected %s' % (name, tuple(out.shape), shape))
    return out, ids


def fused_head_multi_tuple_hist(scores, biases, n, hi, wi, num_classes, groups=None, num_groups=1, hist=None,
                                max_workgroups=0):
    """Two to four experts' low-resolution scores (as fused_head_multi takes them) -> the histogram of their label tuples over
    EVERY output pixel, in one launch and without a label map or ground truth: hist[t] += 1.  Accumulates into hist (int64
    [num_groups, C^E], or [C^E] without groups; made here, zeroed, when None) and returns it.  `groups` as
    fused_head_joint_hist_grouped takes it."""
    scores, biases, E, C, T = _check_tuple_experts(scores, biases, n, hi, wi, num_classes, 'the tuple histogram')
    hist, ids = _grouped_output(hist, 'hist', groups, n, num_groups, (T,), scores[0].device)
    rc = _lib.lib().xv_fused_head_multi_tuple_hist_fwd(_ptr_array(scores), _ptr_array(biases), E, int(n), int(hi), int(wi), C,
                                                      _ptr(ids), int(num_groups), _ptr(hist), int(max_workgroups), _stream())
    _lib.check(rc, 'xv_fused_head_multi_tuple_hist_fwd')
    return hist


def fused_head_multi_lut(scores, biases, n, hi, wi, num_classes, lut, out=None):
    """Two to four experts' low-resolution scores -> the label map (int64 [n, 8hi, 8wi]) a lookup table over their label
    tuples decides, lut uint8 [C^E], in one launch: out = lut[t]."""
    scores, biases, E, C, T = _check_tuple_experts(scores, biases, n, hi, wi, num_classes, 'the lookup head')
    _check_tuple_lut(lut, T)
    out = _label_output(out, n, hi, wi, scores[0].device)
    rc = _lib.lib().xv_fused_head_multi_lut_fwd(_ptr_array(scores), _ptr_array(biases), E, int(n), int(hi), int(wi), C,
                                               _ptr(lut), _ptr(out), _stream())
    _lib.check(rc, 'xv_fused_head_multi_lut_fwd')
    return out


def fused_head_multi_lut_count(scores, biases, n, hi, wi, num_classes, lut, labels, groups=None, num_groups=1, cm=None,
                               max_workgroups=0):
    """Counting form of fused_head_multi_lut: cm[label][lut[t]] += 1 over the pixels with 0 <= label < C (labels int32
    [n, 8hi, 8wi]), without a label map.  Accumulates into cm (int64 [num_groups, C, C], or [C, C] without groups; made here,
    zeroed, when None) and returns it."""
    scores, biases, E, C, T = _check_tuple_experts(scores, biases, n, hi, wi, num_classes, 'the counting lookup head')
    _check_tuple_lut(lut, T)
    _check_labels(labels, n, hi, wi)
    cm, ids = _grouped_output(cm, 'cm', groups, n, num_groups, (C, C), scores[0].device)
    rc = _lib.lib().xv_fused_head_multi_lut_count_fwd(_ptr_array(scores), _ptr_array(biases), E, int(n), int(hi), int(wi), C,
                                                     _ptr(lut), _ptr(labels), _ptr(ids), int(num_groups), _ptr(cm),
                                                     int(max_workgroups), _stream())
    _lib.check(rc, 'xv_fused_head_multi_lut_count_fwd')
    return cm


def fused_head_average_count(Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, labels, cm=None, max_workgroups=0):
    """Both experts' low-resolution scores, average-fused and counted against labels (int32 [n, 8hi, 8wi]): accumulates into cm
    (int64 [C,C], rows = ground truth; made here when None) as confusion_matrix would count fused_head_average's labels, and
    returns it.  No label map is written."""
    C = int(num_classes)
    _check_lowres_pair(Sa, Sb, n, hi, wi, C, labels)
    _need(bias_a, torch.float32, 'bias_a')
    _need(bias_b, torch.float32, 'bias_b')
    if labels.data_ptr() & 15:            # (a slice of a larger map: the kernel reads a pixel group's labels with one load)
        labels = labels.clone()
    if cm is None:
        cm = torch.zeros((C, C), dtype=torch.int64, device=Sa.device)
    _need(cm, torch.int64, 'cm')
    if tuple(cm.shape) != (C, C):
        raise ValueError('cm of shape %s, expected %s' % (tuple(cm.shape), (C, C)))
    rc = _lib.lib().xv_fused_head_average_count_fwd(_ptr(Sa), _ptr(Sb), _ptr(bias_a), _ptr(bias_b), n, hi, wi, C, _ptr(labels),
                                                   _ptr(cm), int(max_workgroups), _stream())
    _lib.check(rc, 'xv_fused_head_average_count_fwd')
    return cm


def variance_head(Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, num_samples, want_score=False, want_probs=False,
                  want_variance=False):
    """Both experts' low-resolution scores of (num_samples + 1) * n images each (slot 0 plain, then the dropout samples) ->
    dict 'label' (int64 [n, 8hi, 8wi]) and, where asked, 'fused_score' (float32 [n, 8hi, 8wi, C]), 'probs' (float32 [2, n,
    8hi, 8wi, C]: the plain passes' softmax) and 'variance' (float32 [2, n, 8hi, 8wi])."""
    for t, name in ((Sa, 'Sa'), (Sb, 'Sb'), (bias_a, 'bias_a'), (bias_b, 'bias_b')):
        _need(t, torch.float32, name)
    T, C = int(num_samples), int(num_classes)
    cp = (C + 3) // 4 * 4
    for t in (Sa, Sb):
        if tuple(t.shape) != ((T + 1) * n, hi + 2, wi + 2, cp):
            raise ValueError('low-resolution scores of shape %s, expected %s' % (tuple(t.shape), ((T + 1) * n, hi + 2, wi + 2, cp)))
    dev, ho, wo = Sa.device, 8 * hi, 8 * wi
    out = {'label': torch.empty((n, ho, wo), dtype=torch.int64, device=dev)}
    if want_score:
        out['fused_score'] = torch.empty((n, ho, wo, C), dtype=torch.float32, device=dev)
    if want_probs:
        out['probs'] = torch.empty((2, n, ho, wo, C), dtype=torch.float32, device=dev)
    if want_variance:
        out['variance'] = torch.empty((2, n, ho, wo), dtype=torch.float32, device=dev)
    rc = _lib.lib().xv_variance_head_fwd(_ptr(Sa), _ptr(Sb), _ptr(bias_a), _ptr(bias_b), n, hi, wi, C, T, _ptr(out['label']),
                                        _ptr(out.get('fused_score')), _ptr(out.get('probs')), _ptr(out.get('variance')),
                                        _stream())
    _lib.check(rc, 'xv_variance_head_fwd')
    return out


def mc_uncertainty_head(S, bias, n, hi, wi, num_classes, num_samples, want_mean=False, want_entropy=False,
                        want_cond_entropy=False, want_variance=False):
    """One expert's low-resolution scores of num_samples * n images (sample-major dropout samples, no plain slot) -> dict
    'label' (int64 [n, 8hi, 8wi]: argmax of the samples' mean softmax) and, where asked, 'mean' (float32 [n, 8hi, 8wi, C]),
    'entropy', 'cond_entropy', 'variance' (float32 [n, 8hi, 8wi]) -- xv_mc_uncertainty_head_fwd."""
    _need(S, torch.float32, 'S')
    _need(bias, torch.float32, 'bias')
    T, C = int(num_samples), int(num_classes)
    cp = (C + 3) // 4 * 4
    if tuple(S.shape) != (T * n, hi + 2, wi + 2, cp):
        raise ValueError('low-resolution scores of shape %s, expected %s' % (tuple(S.shape), (T * n, hi + 2, wi + 2, cp)))
    dev, ho, wo = S.device, 8 * hi, 8 * wi
    out = {'label': torch.empty((n, ho, wo), dtype=torch.int64, device=dev)}
    if want_mean:
        out['mean'] = torch.empty((n, ho, wo, C), dtype=torch.float32, device=dev)
    for key, want in (('entropy', want_entropy), ('cond_entropy', want_cond_entropy), ('variance', want_variance)):
        if want:
            out[key] = torch.empty((n, ho, wo), dtype=torch.float32, device=dev)
    rc = _lib.lib().xv_mc_uncertainty_head_fwd(_ptr(S), _ptr(bias), n, hi, wi, C, T, _ptr(out['label']), _ptr(out.get('mean')),
                                              _ptr(out.get('entropy')), _ptr(out.get('cond_entropy')),
                                              _ptr(out.get('variance')), _stream())
    _lib.check(rc, 'xv_mc_uncertainty_head_fwd')
    return out


UNCERTAINTY_METRICS = ('entropy', 'cond_entropy', 'variance')      # the order of mc_uncertainty_score's histograms


def uncertainty_tables(num_classes, device, num_metrics=1, mantissa_bits=5, octaves=24):
    """Zeroed accumulators of the uncertainty benchmarks: 'hist' (int64 [2, bins], or [num_metrics, 2, bins] for more than one
    metric; bins = octaves << mantissa_bits), 'nll' (float64 [C]) and 'counts' (int64 [C])."""
    bins = int(octaves) << int(mantissa_bits)
    shape = (2, bins) if num_metrics == 1 else (num_metrics, 2, bins)
    return {'hist': torch.zeros(shape, dtype=torch.int64, device=device),
            'nll': torch.zeros(num_classes, dtype=torch.float64, device=device),
            'counts': torch.zeros(num_classes, dtype=torch.int64, device=device)}


def mc_uncertainty_score(S, bias, n, hi, wi, num_classes, num_samples, labels=None, temperature=1.0, fixed_row=-1,
                         mantissa_bits=5, octaves=24, tables=None):
    """The scoring form of mc_uncertainty_head (xv_mc_uncertainty_score_fwd): the same S and bias, logits divided by
    `temperature`; accumulates into `tables` (uncertainty_tables(C, device, 3, ...), made here when None) the histograms of
    entropy, cond_entropy and variance by row -- (label of the mean != labels) over the valid pixels, or `fixed_row` (0 / 1)
    for every pixel -- and, with `labels` (int32 [n, 8hi, 8wi]), the NLL sums and class counts.  Returns the tables."""
    _need(S, torch.float32, 'S')
    _need(bias, torch.float32, 'bias')
    T, C = int(num_samples), int(num_classes)
    cp = (C + 3) // 4 * 4
    if tuple(S.shape) != (T * n, hi + 2, wi + 2, cp):
        raise ValueError('low-resolution scores of shape %s, expected %s' % (tuple(S.shape), (T * n, hi + 2, wi + 2, cp)))
    if labels is not None:
        _need(labels, torch.int32, 'labels')
        if labels.numel() != n * hi * wi * 64:
            raise ValueError('labels of shape %s, expected %s' % (tuple(labels.shape), (n, 8 * hi, 8 * wi)))
    if tables is None:
        tables = uncertainty_tables(C, S.device, 3, mantissa_bits, octaves)
    _check_uncertainty_tables(tables, C, (3, 2, int(octaves) << int(mantissa_bits)))
    rc = _lib.lib().xv_mc_uncertainty_score_fwd(_ptr(S), _ptr(bias), n, hi, wi, C, T, 1.0 / float(temperature), _ptr(labels),
                                               int(mantissa_bits), int(octaves), int(fixed_row), _ptr(tables['hist']),
                                               _ptr(tables['nll']), _ptr(tables['counts']), _stream())
    _lib.check(rc, 'xv_mc_uncertainty_score_fwd')
    return tables


def _check_uncertainty_tables(tables, num_classes, hist_shape):
    _need(tables['hist'], torch.int64, 'hist')
    _need(tables['nll'], torch.float64, 'nll')
    _need(tables['counts'], torch.int64, 'counts')
    if tuple(tables['hist'].shape) != tuple(hist_shape) or tables['nll'].numel() != num_classes or \
            tables['counts'].numel() != num_classes:
        raise ValueError('tables of shapes %s / %s / %s, expected %s and [%d]' % (
            tuple(tables['hist'].shape), tuple(tables['nll'].shape), tuple(tables['counts'].shape), tuple(hist_shape),
            num_classes))


def uncertainty_stats(metric, pred, labels, num_classes, mean_prob=None, fixed_row=-1, mantissa_bits=5, octaves=24,
                      tables=None):
    """The benchmarks' statistic on materialised maps (xv_uncertainty_stats): metric float32 [...] (one uncertainty map), pred
    int64 [...] and labels int32 [...] (both may be None with a fixed row).  Accumulates into `tables`
    (uncertainty_tables(C, device), made here when None) hist[row][bin(metric)] with row = (pred != labels) over the valid
    pixels or `fixed_row` for every pixel, and, with mean_prob (float32 [..., C]), the NLL sums and class counts.  Returns the
    tables."""
    _need(metric, torch.float32, 'metric')
    if pred is not None:
        _need(pred, torch.int64, 'pred')
    if labels is not None:
        _need(labels, torch.int32, 'labels')
    if mean_prob is not None:
        _need(mean_prob, torch.float32, 'mean_prob')
    C, npix = int(num_classes), metric.numel()
    for t, want in ((pred, npix), (labels, npix), (mean_prob, npix * C)):
        if t is not None and t.numel() != want:
            raise ValueError('maps of different sizes')
    if tables is None:
        tables = uncertainty_tables(C, metric.device, 1, mantissa_bits, octaves)
    _check_uncertainty_tables(tables, C, (2, int(octaves) << int(mantissa_bits)))
    rc = _lib.lib().xv_uncertainty_stats(_ptr(metric), _ptr(pred), _ptr(labels), _ptr(mean_prob), C, npix, int(mantissa_bits),
                                        int(octaves), int(fixed_row), _ptr(tables['hist']), _ptr(tables['nll']),
                                        _ptr(tables['counts']), _stream())
    _lib.check(rc, 'xv_uncertainty_stats')
    return tables


def sampling_uncertainty(samples, want_label=True, want_mean=True, want_entropy=True, want_cond_entropy=True,
                         want_variance=True):
    """bayesian_fcn.py:48-57 on materialised samples float32 [T, ..., C] (xv_sampling_uncertainty) -> dict with the asked of
    'label' (int64 [...]), 'mean' (float32 [..., C]), 'entropy', 'cond_entropy', 'variance' (float32 [...])."""
    _need(samples, torch.float32, 'samples')
    if samples.dim() < 3:
        raise ValueError('samples of shape [T, ..., C]')
    T, c = samples.shape[0], samples.shape[-1]
    shape = tuple(samples.shape[1:-1])
    dev = samples.device
    out = {}
    if want_label:
        out['label'] = torch.empty(shape, dtype=torch.int64, device=dev)
    if want_mean:
        out['mean'] = torch.empty(shape + (c,), dtype=torch.float32, device=dev)
    for key, want in (('entropy', want_entropy), ('cond_entropy', want_cond_entropy), ('variance', want_variance)):
        if want:
            out[key] = torch.empty(shape, dtype=torch.float32, device=dev)
    rc = _lib.lib().xv_sampling_uncertainty(_ptr(samples), T, c, samples.numel() // (T * c), _ptr(out.get('label')),
                                           _ptr(out.get('mean')), _ptr(out.get('entropy')), _ptr(out.get('cond_entropy')),
                                           _ptr(out.get('variance')), _stream())
    _lib.check(rc, 'xv_sampling_uncertainty')
    return out


def dropout_pixels_samples(x, num_samples, rate, seed0, stride, plain=True, y=None):
    """Input dropout of whole pixels (xv_dropout_pixels_samples): x float32 [n, h, w, cin] -> float32 [(plain + T) n, h, w,
    cin], slot-major -- slot 0 = x when `plain`, sample t = 0 .. T-1 = dropout_pixels(x, rate, seed0 + t * stride)."""
    _need(x, torch.float32, 'x')
    if x.dim() != 4:
        raise ValueError('x of shape [n, h, w, cin]')
    T = int(num_samples)
    n, h, w, cin = x.shape
    shape = ((T + int(bool(plain))) * n, h, w, cin)
    if y is None:
        y = torch.empty(shape, dtype=torch.float32, device=x.device)
    _need(y, torch.float32, 'y')
    if tuple(y.shape) != shape:
        raise ValueError('y of shape %s, expected %s' % (tuple(y.shape), shape))
    rc = _lib.lib().xv_dropout_pixels_samples(_ptr(x), n, h, w, cin, _ptr(y), T, int(bool(plain)), float(rate),
                                             int(seed0) & 0xffffffffffffffff, int(stride) & 0xffffffffffffffff, _stream())
    _lib.check(rc, 'xv_dropout_pixels_samples')
    return y


def dropout_pixels(x, rate, seed, y=None):
    """tf.layers.dropout(x, rate, noise_shape=[N, H, W, 1], training=True) on the dense float32 input: one draw per pixel,
    shared by its channels; kept pixels scaled by 1 / (1 - rate)."""
    return dropout_pixels_samples(x, 1, rate, seed, 0, plain=False, y=y)


def uncertainty_moments(Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, num_samples):
    """Both experts' low-resolution scores of (num_samples + 1) * n images each (slot 0 plain, then the samples) -> (mvar float32
    [2, n, 8hi, 8wi]: the samples' population variance averaged over the classes, the bits of variance_head's 'variance'; vmax
    float32 [2]: each expert's largest per-class variance over the whole call)."""
    for t, name in ((Sa, 'Sa'), (Sb, 'Sb'), (bias_a, 'bias_a'), (bias_b, 'bias_b')):
        _need(t, torch.float32, name)
    T, C = int(num_samples), int(num_classes)
    cp = (C + 3) // 4 * 4
    for t in (Sa, Sb):
        if tuple(t.shape) != ((T + 1) * n, hi + 2, wi + 2, cp):
            raise ValueError('low-resolution scores of shape %s, expected %s' % (tuple(t.shape), ((T + 1) * n, hi + 2, wi + 2, cp)))
    mvar = torch.empty((2, n, 8 * hi, 8 * wi), dtype=torch.float32, device=Sa.device)
    vmax = torch.empty(2, dtype=torch.float32, device=Sa.device)
    rc = _lib.lib().xv_uncertainty_moments(_ptr(Sa), _ptr(Sb), _ptr(bias_a), _ptr(bias_b), n, hi, wi, C, T, _ptr(mvar),
                                          _ptr(vmax), _stream())
    _lib.check(rc, 'xv_uncertainty_moments')
    return mvar, vmax


def uncertainty_dirichlet_head(Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, mvar, vmax, params, logprior, want_score=False,
                               want_probs=False, want_mix=False):
    """The plain slots of both experts' low-resolution scores (any number of slots behind them), mvar / vmax of
    uncertainty_moments, params float32 [2, C, C] (params[e, j, c]) and logprior float32 [C] -> dict 'label' (int64 [n, 8hi,
    8wi]) and, where asked, 'fused_score' (float32 [n, 8hi, 8wi, C]), 'probs' (float32 [2, n, 8hi, 8wi, C]) and 'mix' (float32
    [2, n, 8hi, 8wi])."""
    for t, name in ((Sa, 'Sa'), (Sb, 'Sb'), (bias_a, 'bias_a'), (bias_b, 'bias_b'), (mvar, 'mvar'), (vmax, 'vmax'),
                    (params, 'params'), (logprior, 'logprior')):
        _need(t, torch.float32, name)
    C = int(num_classes)
    cp = (C + 3) // 4 * 4
    for t in (Sa, Sb):
        if t.dim() != 4 or t.shape[0] < n or tuple(t.shape[1:]) != (hi + 2, wi + 2, cp):
            raise ValueError('low-resolution scores of shape %s, expected at least %s' % (tuple(t.shape), (n, hi + 2, wi + 2, cp)))
    dev, ho, wo = Sa.device, 8 * hi, 8 * wi
    if tuple(mvar.shape) != (2, n, ho, wo) or vmax.numel() != 2 or tuple(params.shape) != (2, C, C) or logprior.numel() != C:
        raise ValueError('mvar [2, n, 8hi, 8wi], vmax [2], params [2, C, C] and logprior [C]')
    out = {'label': torch.empty((n, ho, wo), dtype=torch.int64, device=dev)}
    if want_score:
        out['fused_score'] = torch.empty((n, ho, wo, C), dtype=torch.float32, device=dev)
    if want_probs:
        out['probs'] = torch.empty((2, n, ho, wo, C), dtype=torch.float32, device=dev)
    if want_mix:
        out['mix'] = torch.empty((2, n, ho, wo), dtype=torch.float32, device=dev)
    rc = _lib.lib().xv_uncertainty_dirichlet_head_fwd(_ptr(Sa), _ptr(Sb), _ptr(bias_a), _ptr(bias_b), n, hi, wi, C, _ptr(mvar),
                                                     _ptr(vmax), _ptr(params), _ptr(logprior), _ptr(out['label']),
                                                     _ptr(out.get('fused_score')), _ptr(out.get('probs')), _ptr(out.get('mix')),
                                                     _stream())
    _lib.check(rc, 'xv_uncertainty_dirichlet_head_fwd')
    return out


def uncertainty_dirichlet_fuse(probs, mvar, vmax, params, logprior, want_score=True, want_label=True):
    """uncertainty_dirichlet_mix.py:18-52 on two experts: probs float32 [..., C] each, mvar float32 [2, ...], vmax float32 [2],
    params float32 [2, C, C], logprior float32 [C] -> (fused label int64 [...] or None, fused score float32 [..., C] or None)."""
    for t, name in ((mvar, 'mvar'), (vmax, 'vmax'), (params, 'params'), (logprior, 'logprior')) + tuple((p, 'probs') for p in probs):
        _need(t, torch.float32, name)
    if len(probs) != 2:
        raise ValueError('two experts')
    c = probs[0].shape[-1]
    shape = tuple(probs[0].shape[:-1])
    if tuple(probs[1].shape) != shape + (c,) or tuple(mvar.shape) != (2,) + shape or vmax.numel() != 2 or \
            tuple(params.shape) != (2, c, c) or logprior.numel() != c:
        raise ValueError('probs [..., C] twice, mvar [2, ...], vmax [2], params [2, C, C] and logprior [C]')
    dev = probs[0].device
    fused = torch.empty(shape, dtype=torch.int64, device=dev) if want_label else None
    score = torch.empty(shape + (c,), dtype=torch.float32, device=dev) if want_score else None
    rc = _lib.lib().xv_uncertainty_dirichlet_fuse(_ptr_array(probs), _ptr(mvar), _ptr(vmax), _ptr(params), _ptr(logprior), c,
                                                 probs[0].numel() // c, _ptr(fused), _ptr(score), _stream())
    _lib.check(rc, 'xv_uncertainty_dirichlet_fuse')
    return fused, score


def uncertainty_weights(unc, mvar=None, vmax=None):
    """One expert's per-class uncertainties float32 [..., C] (non-negative) -> (mvar float32 [...], their class mean; vmax
    float32 [1], their maximum over everything).  mvar / vmax: views to write into (one expert's part of a [2, ...] pair)."""
    _need(unc, torch.float32, 'unc')
    c = unc.shape[-1]
    if mvar is None:
        mvar = torch.empty(tuple(unc.shape[:-1]), dtype=torch.float32, device=unc.device)
    if vmax is None:
        vmax = torch.empty(1, dtype=torch.float32, device=unc.device)
    _need(mvar, torch.float32, 'mvar')
    _need(vmax, torch.float32, 'vmax')
    if mvar.numel() * c != unc.numel() or vmax.numel() != 1:
        raise ValueError('mvar of one value per pixel and vmax of one value')
    rc = _lib.lib().xv_uncertainty_weights(_ptr(unc), c, unc.numel() // c, _ptr(mvar), _ptr(vmax), _stream())
    _lib.check(rc, 'xv_uncertainty_weights')
    return mvar, vmax


def softmax_argmax(score, want_prob=True, want_label=True):
    _need(score, torch.float32, 'score')
    c = score.shape[-1]
    npix = score.numel() // c
    prob = torch.empty_like(score) if want_prob else None
    label = torch.empty(score.shape[:-1], dtype=torch.int64, device=score.device) if want_label else None
    _lib.check(_lib.lib().xv_softmax_argmax(_ptr(score), npix, c, _ptr(prob), _ptr(label), _stream()), 'xv_softmax_argmax')
    return prob, label


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def bayes_fuse(labels, loglik, logprior, want_score=False):
    """labels: list of int64 tensors (same shape); loglik float32 [E,C,C]; logprior float32 [C]."""
    for l in labels:
        _need(l, torch.int64, 'labels')
    _need(loglik, torch.float32, 'loglik')
    _need(logprior, torch.float32, 'logprior')
    e, c = loglik.shape[0], loglik.shape[1]
    npix = labels[0].numel()
    fused = torch.empty_like(labels[0])
    score = torch.empty(tuple(labels[0].shape) + (c,), dtype=torch.float32, device=fused.device) if want_score else None
    rc = _lib.lib().xv_bayes_fuse(_ptr_array(labels), e, _ptr(loglik), _ptr(logprior), c, npix, _ptr(fused), _ptr(score), _stream())
    _lib.check(rc, 'xv_bayes_fuse')
    return fused, score


def bayes_fuse_lut(label_a, label_b, lut):
    _need(label_a, torch.int64, 'label_a')
    _need(label_b, torch.int64, 'label_b')
    _need(lut, torch.int64, 'lut')
    fused = torch.empty_like(label_a)
    rc = _lib.lib().xv_bayes_fuse_lut(_ptr(label_a), _ptr(label_b), _ptr(lut), lut.shape[0], label_a.numel(), _ptr(fused), _stream())
    _lib.check(rc, 'xv_bayes_fuse_lut')
    return fused


def dirichlet_fuse(probs, am1, lognorm, logprior, want_score=False):
    for p in probs:
        _need(p, torch.float32, 'probs')
    e, c = am1.shape[0], am1.shape[1]
    npix = probs[0].numel() // c
    fused = torch.empty(probs[0].shape[:-1], dtype=torch.int64, device=probs[0].device)
    score = torch.empty_like(probs[0]) if want_score else None
    rc = _lib.lib().xv_dirichlet_fuse(_ptr_array(probs), e, _ptr(am1), _ptr(lognorm), _ptr(logprior), c, npix,
                                     _ptr(fused), _ptr(score), _stream())
    _lib.check(rc, 'xv_dirichlet_fuse')
    return fused, score


def average_fuse(probs):
    for p in probs:
        _need(p, torch.float32, 'probs')
    c = probs[0].shape[-1]
    fused = torch.empty(probs[0].shape[:-1], dtype=torch.int64, device=probs[0].device)
    rc = _lib.lib().xv_average_fuse(_ptr_array(probs), len(probs), c, probs[0].numel() // c, _ptr(fused), _stream())
    _lib.check(rc, 'xv_average_fuse')
    return fused


def variance_fuse(probs, variances, want_score=True, want_label=True):
    """variance_mix.py:7-15 on E experts: probs float32 [..., C] each, variances float32 [...] (one per pixel) -> (fused label
    int64 [...] or None, fused score float32 [..., C] or None)."""
    for p in probs:
        _need(p, torch.float32, 'probs')
    for v in variances:
        _need(v, torch.float32, 'variances')
    if len(probs) != len(variances) or not probs:
        raise ValueError('one variance map per probability map')
    c = probs[0].shape[-1]
    shape = tuple(probs[0].shape[:-1])
    if any(tuple(p.shape) != shape + (c,) for p in probs) or any(tuple(v.shape) != shape for v in variances):
        raise ValueError('probability maps [..., C] and variance maps [...] of one shape')
    dev = probs[0].device
    fused = torch.empty(shape, dtype=torch.int64, device=dev) if want_label else None
    score = torch.empty(shape + (c,), dtype=torch.float32, device=dev) if want_score else None
    rc = _lib.lib().xv_variance_fuse(_ptr_array(probs), _ptr_array(variances), len(probs), c, probs[0].numel() // c,
                                    _ptr(fused), _ptr(score), _stream())
    _lib.check(rc, 'xv_variance_fuse')
    return fused, score


def dirichlet_suffstats(prob, labels, S, counts):
    """Accumulates into S (float64 [C,C]) and counts (int64 [C]) in place."""
    _need(prob, torch.float32, 'prob')
    _need(labels, torch.int32, 'labels')
    _need(S, torch.float64, 'S')
    _need(counts, torch.int64, 'counts')
    c = prob.shape[-1]
    rc = _lib.lib().xv_dirichlet_suffstats(_ptr(prob), _ptr(labels), c, labels.numel(), _ptr(S), _ptr(counts), _stream())
    _lib.check(rc, 'xv_dirichlet_suffstats')


def confusion_matrix(labels, pred, cm):
    """Accumulates into cm (int64 [C,C], rows = ground truth) in place."""
    _need(labels, torch.int32, 'labels')
    _need(pred, torch.int64, 'pred')
    _need(cm, torch.int64, 'cm')
    rc = _lib.lib().xv_confusion_matrix(_ptr(labels), _ptr(pred), cm.shape[0], labels.numel(), _ptr(cm), _stream())
    _lib.check(rc, 'xv_confusion_matrix')


def confusion_matrix_grouped(labels, pred, groups, num_groups, cm=None, num_classes=None):
    """confusion_matrix per group of images: labels int32 / pred int64 [n, ...] with the image axis first, `groups` one id in
    [0, num_groups) per image (host side: checked here before anything is launched; or a device slice of upload_group_ids'
    result).  Accumulates into cm (int64 [G,C,C], rows = ground truth) and returns it; with cm=None a zeroed one is made here,
    for which the class count has to be named: `num_classes` (the maps do not carry it)."""
    _need(labels, torch.int32, 'labels')
    _need(pred, torch.int64, 'pred')
    G = int(num_groups)
    if labels.dim() < 2 or labels.shape != pred.shape or labels.numel() == 0:
        raise ValueError('labels %s and pred %s must be equal non-empty shapes [n, ...]' % (tuple(labels.shape), tuple(pred.shape)))
    n = labels.shape[0]
    ids = _group_ids(groups, n, G, labels.device)
    if cm is None:
        if num_classes is None:
            raise ValueError('confusion_matrix_grouped makes cm itself only when told num_classes')
        cm = torch.zeros((G, int(num_classes), int(num_classes)), dtype=torch.int64, device=labels.device)
    _need(cm, torch.int64, 'cm')
    if cm.dim() != 3 or cm.shape[0] != G or cm.shape[1] != cm.shape[2] or (num_classes is not None and cm.shape[1] != num_classes):
        raise ValueError('cm of shape %s, expected [%d, C, C]' % (tuple(cm.shape), G))
    rc = _lib.lib().xv_confusion_matrix_grouped(_ptr(labels), _ptr(pred), _ptr(ids), n, labels.numel() // n, cm.shape[1], G,
                                               _ptr(cm), _stream())
    _lib.check(rc, 'xv_confusion_matrix_grouped')
    return cm


# ---- training ----------------------------------------------------------------------------------------

def pack_conv_weights_dgrad(w_hwio, out=None):
    """float32 HWIO device tensor -> packed bf16 weights of the data-gradient convolution."""
    _need(w_hwio, torch.float32, 'w_hwio')
    k, _, cin, cout = w_hwio.shape
    if out is None:
        out = torch.empty(_lib.lib().xv_packed_weight_bytes(k, cout, cin) // 2, dtype=torch.bfloat16, device=w_hwio.device)
    _lib.check(_lib.lib().xv_pack_conv_weights_dgrad(_ptr(w_hwio), _ptr(out), k, cin, cout, _stream()),
               'xv_pack_conv_weights_dgrad')
    return out


def pack_conv_weights_into(w_hwio, out):
    k, _, cin, cout = w_hwio.shape
    _lib.check(_lib.lib().xv_pack_conv_weights(_ptr(w_hwio), _ptr(out), k, cin, cout, _stream()), 'xv_pack_conv_weights')
    return out


def pack_conv_weights_pair(w_hwio, out, out_dgrad):
    """Forward and data-gradient packed images of one kernel in one launch."""
    _need(w_hwio, torch.float32, 'w_hwio')
    k, _, cin, cout = w_hwio.shape
    _lib.check(_lib.lib().xv_pack_conv_weights_pair(_ptr(w_hwio), _ptr(out), _ptr(out_dgrad), k, cin, cout, _stream()),
               'xv_pack_conv_weights_pair')


class PackTable(object):
    """Descriptor table (in device memory) of every (master kernel, packed forward image, packed data-gradient image)
    triple of a trainer; run() re-packs them all in ONE launch.  The tensors must stay where they are."""

    def __init__(self, entries, device):
        """entries: list of (w_hwio float32 [k,k,cin,cout] view, packed bf16 buffer, packed dgrad bf16 buffer or None)."""
        self.keep = list(entries)
        arr = (_lib.xv_pack_desc * len(entries))()
        for i, (w, out, outd) in enumerate(entries):
            _need(w, torch.float32, 'w_hwio')
            k, _, cin, cout = w.shape
            arr[i] = _lib.xv_pack_desc(w.data_ptr(), out.data_ptr(), outd.data_ptr() if outd is not None else None, k, cin, cout, 0)
        raw = bytes(arr)
        self.table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        self.n = len(entries)

    def run(self):
        _lib.check(_lib.lib().xv_pack_conv_weights_multi(_ptr(self.table), self.n, _stream()), 'xv_pack_conv_weights_multi')


def zero_(t):
    """Clear a tensor on the current stream with the library's memset (no framework kernel in the training step)."""
    _lib.check(_lib.lib().xv_memset_zero(_ptr(t), t.numel() * t.element_size(), _stream()), 'xv_memset_zero')
    return t


class _Profiled(object):
    """with _Profiled(kind, flops): ... -- a HIP-event pair on the launch stream when bench.py collects CONV_PROFILE."""

    def __init__(self, kind, flops):
        self.kind, self.flops, self.prof = kind, flops, CONV_PROFILE

    def __enter__(self):
        if self.prof is not None:
            self.ev0, self.ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.ev0.record()

    def __exit__(self, *exc):
        if self.prof is not None:
            self.ev1.record()
            self.prof.append((self.kind, self.flops, self.ev0, self.ev1))


def conv2d_bwd_data(dy, w_packed_dgrad, zero_bias, dx, k, relu_ref=None, addend=None, workspace=None):
    with _Profiled('dgrad_k%d' % k, 2.0 * dx.n * dx.h * dx.w * dx.c * dy.c * k * k):
        if workspace is None:
            rc = _lib.lib().xv_conv2d_bwd_data(dy.xv(), _ptr(w_packed_dgrad), _ptr(zero_bias),
                                              relu_ref.xv() if relu_ref is not None else _NULL_ACT,
                                              addend.xv() if addend is not None else _NULL_ACT, dx.xv(), k, _stream())
        else:
            rc = _lib.lib().xv_conv2d_bwd_data_ws(dy.xv(), _ptr(w_packed_dgrad), _ptr(zero_bias),
                                                 relu_ref.xv() if relu_ref is not None else _NULL_ACT,
                                                 addend.xv() if addend is not None else _NULL_ACT, dx.xv(), k,
                                                 _ptr(workspace), workspace.numel() * workspace.element_size(), _stream())
    _lib.check(rc, 'xv_conv2d_bwd_data')
    return dx


def conv2d_bwd_filter_workspace_bytes(x, cout, k):
    return _lib.lib().xv_conv2d_bwd_filter_workspace_bytes(x.n, x.h, x.w, x.c, cout, k)


def conv2d_bwd_filter(x, dy, dw, dbias, k, workspace=None):
    """workspace (float32 tensor of >= conv2d_bwd_filter_workspace_bytes): every partial sum (the pixel splits of dW and
    of the bias gradient) goes to slabs added in a fixed order -- bitwise reproducible; None: fp32 atomics."""
    _need(dw, torch.float32, 'dw')
    with _Profiled('wgrad_k%d' % k, 2.0 * x.n * x.h * x.w * x.c * dy.c * k * k):
        if workspace is None:
            rc = _lib.lib().xv_conv2d_bwd_filter(x.xv(), dy.xv(), _ptr(dw), _ptr(dbias), k, _stream())
        else:
            rc = _lib.lib().xv_conv2d_bwd_filter_ws(x.xv(), dy.xv(), _ptr(dw), _ptr(dbias), k, _ptr(workspace),
                                                   workspace.numel() * 4, _stream())
    _lib.check(rc, 'xv_conv2d_bwd_filter')


def conv2d_first_bwd_filter(x, dy, dw, dbias=None, workspace=None):
    """workspace (float32 tensor of >= conv2d_first_bwd_filter_workspace_bytes): per-workgroup partial sums + a
    fixed-order reduce (bitwise reproducible; needs dbias); None: fp32 atomics."""
    _need(x, torch.float32, 'x')
    n, h, w, cin = x.shape
    if workspace is None or dbias is None:
        rc = _lib.lib().xv_conv2d_first_bwd_filter(_ptr(x), n, h, w, cin, dy.xv(), _ptr(dw), _ptr(dbias), _stream())
    else:
        rc = _lib.lib().xv_conv2d_first_bwd_filter_ws(_ptr(x), n, h, w, cin, dy.xv(), _ptr(dw), _ptr(dbias), _ptr(workspace),
                                                      workspace.numel() * 4, _stream())
    _lib.check(rc, 'xv_conv2d_first_bwd_filter')


def conv2d_first_bwd_filter_workspace_bytes(x):
    n, h, w, cin = x.shape
    return _lib.lib().xv_conv2d_first_bwd_filter_workspace_bytes(n, h, w, cin)


def maxpool2x2_bwd(y, dpooled, dy):
    _lib.check(_lib.lib().xv_maxpool2x2_bwd(y.xv(), dpooled.xv(), dy.xv(), _stream()), 'xv_maxpool2x2_bwd')
    return dy


ROUTED_POOL = True     # False (a test seam): full maps + xv_maxpool2x2_bwd everywhere -- the same bits


def conv2d_fwd_route(x, w_packed, bias, pooled, route):
    """pooled = maxpool2x2(relu(conv3x3(x) + bias)) and its route bytes (uint8 tensor of >= n * h/2 * w/2 * cout elements) in
    one launch, no full map (xv_conv2d_fwd_route).  Returns False -- nothing launched -- where the generation-4 kernel does not
    take the shape: the caller then writes the full map (conv2d_fwd) and routes with maxpool2x2_bwd."""
    # (the data-gradient conv that reads the routes runs at the POOLED size: that must tile in 16x32 pixels too)
    if not ROUTED_POOL or x.dtype != 'bf16' or x.h % 32 or x.w % 64:
        return False
    _need(bias, torch.float32, 'bias')
    _need(route, torch.uint8, 'route')
    with _Profiled('k3', 2.0 * x.n * x.h * x.w * x.c * pooled.c * 9):
        rc = _lib.lib().xv_conv2d_fwd_route(x.xv(), _ptr(w_packed), _ptr(bias), pooled.xv(), _ptr(route), route.numel(), _stream())
    if rc == XV_ESHAPE:
        return False
    _lib.check(rc, 'xv_conv2d_fwd_route')
    return True


def conv2d_bwd_data_route(dy, w_packed_dgrad, zero_bias, route, dx):
    """dx (twice dy's size) = MaxPoolGrad + ReluGrad of conv3x3(dy, Wd) through the route bytes of conv2d_fwd_route: the bits
    of conv2d_bwd_data onto a pooled-size map + maxpool2x2_bwd, without either map in memory."""
    _need(route, torch.uint8, 'route')
    with _Profiled('dgrad_k3', 2.0 * dy.n * dy.h * dy.w * dx.c * dy.c * 9):
        rc = _lib.lib().xv_conv2d_bwd_data_route(dy.xv(), _ptr(w_packed_dgrad), _ptr(zero_bias), _ptr(route), route.numel(),
                                                 dx.xv(), _stream())
    _lib.check(rc, 'xv_conv2d_bwd_data_route')
    return dx


def relu_bwd(g, ref, out):
    _lib.check(_lib.lib().xv_relu_bwd(g.xv(), ref.xv(), out.xv(), _stream()), 'xv_relu_bwd')
    return out


def upsample2x_bwd(dfused, s5, ds5):
    _lib.check(_lib.lib().xv_upsample2x_bwd(dfused.xv(), s5.xv(), ds5.xv(), _stream()), 'xv_upsample2x_bwd')
    return ds5


def count_valid_labels(labels, num_classes, count):
    _need(labels, torch.int32, 'labels')
    _need(count, torch.int64, 'count')
    _lib.check(_lib.lib().xv_count_valid_labels(_ptr(labels), num_classes, labels.numel(), _ptr(count), _stream()),
               'xv_count_valid_labels')


def decoder_head_bwd(fused, w_score, b_score, labels, count, num_classes, loss, dw_score, db_score, dfused,
                     workspace=None):
    _need(labels, torch.int32, 'labels')
    _need(loss, torch.float64, 'loss')
    if workspace is None:
        nbytes = _lib.lib().xv_decoder_head_bwd_workspace_bytes(fused.n, fused.h, fused.w, num_classes)
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=fused.t.device)
    rc = _lib.lib().xv_decoder_head_bwd(fused.xv(), _ptr(w_score), _ptr(b_score), _ptr(labels), _ptr(count), num_classes,
                                       _ptr(loss), _ptr(dw_score), _ptr(db_score), dfused.xv(), _ptr(workspace),
                                       workspace.numel() * 4, _stream())
    _lib.check(rc, 'xv_decoder_head_bwd')
    return workspace


def adam_step(param, grad, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _lib.check(_lib.lib().xv_adam_step(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), param.numel(), lr_t, beta1, beta2, eps,
                                      grad_scale, _stream()), 'xv_adam_step')


def rmsprop_step(param, grad, ms, lr, decay=0.9, eps=1e-10, grad_scale=1.0):
    _lib.check(_lib.lib().xv_rmsprop_step(_ptr(param), _ptr(grad), _ptr(ms), param.numel(), lr, decay, eps, grad_scale,
                                         _stream()), 'xv_rmsprop_step')


def adagrad_step(param, grad, accum, lr, grad_scale=1.0):
    _lib.check(_lib.lib().xv_adagrad_step(_ptr(param), _ptr(grad), _ptr(accum), param.numel(), lr, grad_scale, _stream()),
               'xv_adagrad_step')


def bias_grad(dy, dbias):
    _need(dbias, torch.float32, 'dbias')
    _lib.check(_lib.lib().xv_bias_grad(dy.xv(), _ptr(dbias), _stream()), 'xv_bias_grad')


# ---- training-mode batch norm and the un-commuted training head (csrc/batchnorm.hip) -------------------------
BN_EPS, BN_MOMENTUM = 1e-3, 0.99        # [TF1] tf.layers.batch_normalization defaults


class BnState(object):
    """Per-layer buffers of one training-mode batch norm: batch statistics, folded scale / shift, scratch."""

    def __init__(self, channels, device, deterministic=True):
        f = lambda: torch.zeros(channels, dtype=torch.float32, device=device)   # noqa: E731
        self.c = channels
        self.mean, self.invstd, self.scale, self.shift = f(), f(), f(), f()
        self.sums = torch.zeros(2 * channels, dtype=torch.float64, device=device)
        # per-workgroup partial sums of the reductions, added in a fixed order (xv_bn_workspace_bytes): bitwise
        # reproducible statistics and gamma / beta gradients; deterministic=False: f64 atomics in arrival order
        self.ws = torch.empty(_lib.lib().xv_bn_workspace_bytes(channels) // 4, dtype=torch.float32, device=device) \
            if deterministic else None

    def wsp(self):
        return (_ptr(self.ws), self.ws.numel() * 4) if self.ws is not None else (None, 0)


def _sync_sums(st, sync):
    """Sync-BN: sum the per-channel statistics over the data-parallel ranks; returns the factor by which the local
    sample count grows.  Every rank holds the same number of images per step: the models check that the ranks agree on
    `batchsize` when the trainer is created and that every data-parallel step has exactly that many images
    (parallel.require_equal_batchsize)."""
    if not sync:
        return 1
    from .parallel import allreduce_stats_, world
    allreduce_stats_(st.sums)           # on a communicator of its own: never queued behind a gradient bucket in flight
    return world()[1]


def conv2d_fwd_stats(x, w_packed, bias, z, st):
    """z = conv3x3(x) + bias with the batch statistics of z taken in the conv kernel's epilogue -- as PER-WORKGROUP ROWS in
    st.conv_rows (st.conv_rows_n of them), NOT in st.sums: the sums are produced by the next bn_forward(have_stats=True)
    (xv_bn_finalize_from_rows / xv_bn_sums_from_rows), until then st.sums still holds the previous step's values.  Returns
    False (nothing launched) where that kernel does not apply: the caller then runs conv2d_fwd and lets bn_forward take the
    statistics."""
    lib = _lib.lib()
    rows = lib.xv_conv2d_stats_rows()
    if getattr(st, 'conv_rows', None) is None or st.conv_rows.numel() < rows * 2 * st.c:
        st.conv_rows = torch.empty(rows * 2 * st.c, dtype=torch.float32, device=z.t.device)
    rc = lib.xv_conv2d_fwd_stats(x.xv(), _ptr(w_packed), _ptr(bias), z.xv(), _ptr(st.conv_rows), st.conv_rows.numel() * 4,
                                 _stream())
    if rc == XV_ESHAPE:     # the generation-4 kernel does not take this shape
        return False
    _lib.check(rc, 'xv_conv2d_fwd_stats')
    st.conv_rows_n = rows       # bn_forward(have_stats=True) adds the rows up (in the launch that finalises, where it can)
    return True


def bn_forward(z, gamma, beta, moving_mean, moving_var, st, y, relu=True, sync=False, pooled=None, have_stats=False,
               ups8_of=None):
    """y = [relu](BN_batch(z)); updates the moving statistics in place (z, y: Act).  sync: statistics over all
    data-parallel ranks (one all-reduce of 2*C doubles).  pooled (with relu): the 2x2 max-pool of y from the same pass; y
    may then be None (only the pooled map is written).  ups8_of (an Act 8 times smaller, with z None): z IS its bilinear x8
    up-sampling and is recomputed per element instead of read (deterministic workspace only; with sync the sums are all-reduced
    between the statistics pass and the per-channel results, like every other batch norm)."""
    lib = _lib.lib()
    fin = (_ptr(gamma), _ptr(beta), BN_EPS, BN_MOMENTUM, _ptr(moving_mean), _ptr(moving_var), _ptr(st.mean), _ptr(st.invstd),
           _ptr(st.scale), _ptr(st.shift))
    ws = st.wsp()
    if ups8_of is not None:
        if st.ws is None or pooled is not None or have_stats:
            raise ValueError('bn_forward(ups8_of=): statistics with a workspace, no pool')
        if sync:    # data parallel: the sums alone, all-reduced over the ranks, then the per-channel results
            _lib.check(lib.xv_bn_stats_ups8_ws(ups8_of.xv(), _ptr(st.sums), ws[0], ws[1], _stream()), 'xv_bn_stats_ups8_ws')
            mult = _sync_sums(st, sync)
            _lib.check(lib.xv_bn_finalize(_ptr(st.sums), st.c, ups8_of.n * 64 * ups8_of.h * ups8_of.w * mult, *fin, _stream()),
                       'xv_bn_finalize')
        else:
            _lib.check(lib.xv_bn_stats_finalize_ups8_ws(ups8_of.xv(), _ptr(st.sums), ws[0], ws[1], *fin, _stream()),
                       'xv_bn_stats_finalize_ups8_ws')
        if y is None:           # statistics only: the apply pass is fused into what follows (score_dense_fwd_ups8)
            return None
        _lib.check(lib.xv_bn_apply_ups8(ups8_of.xv(), _ptr(st.scale), _ptr(st.shift), int(bool(relu)), y.xv(), _stream()),
                   'xv_bn_apply_ups8')
        return y
    if not sync and have_stats:
        # one process: the row sums of the conv epilogue's partial statistics and the per-channel results in ONE launch
        _lib.check(lib.xv_bn_finalize_from_rows(_ptr(st.conv_rows), st.conv_rows_n, st.c, z.n * z.h * z.w, *fin, _ptr(st.sums),
                                                _stream()), 'xv_bn_finalize_from_rows')
    elif not sync and st.ws is not None:
        _lib.check(lib.xv_bn_stats_finalize_ws(z.xv(), _ptr(st.sums), ws[0], ws[1], *fin, _stream()), 'xv_bn_stats_finalize_ws')
    else:
        if have_stats:
            _lib.check(lib.xv_bn_sums_from_rows(_ptr(st.conv_rows), st.conv_rows_n, 2 * st.c, _ptr(st.sums), _stream()),
                       'xv_bn_sums_from_rows')
        else:
            _lib.check(lib.xv_bn_stats_ws(z.xv(), _ptr(st.sums), *ws, _stream()), 'xv_bn_stats_ws')
        mult = _sync_sums(st, sync)
        _lib.check(lib.xv_bn_finalize(_ptr(st.sums), st.c, z.n * z.h * z.w * mult, *fin, _stream()), 'xv_bn_finalize')
    if pooled is not None:
        if not relu:
            raise ValueError('the fused pool follows the relu')
        _lib.check(lib.xv_bn_apply_pool(z.xv(), _ptr(st.scale), _ptr(st.shift), y.xv() if y is not None else _NULL_ACT,
                                        pooled.xv(), _stream()), 'xv_bn_apply_pool')
        return y
    _lib.check(lib.xv_bn_apply(z.xv(), _ptr(st.scale), _ptr(st.shift), int(bool(relu)), y.xv(), _stream()), 'xv_bn_apply')
    return y


def bn_backward(dy, y, z, gamma, st, dgamma, dbeta, dz, sync=False, mask_from_z=None, relu=None, ups8_of=None):
    """dz from dy (gradient w.r.t. the post-relu output); accumulates the LOCAL dgamma / dbeta (the gradient all-reduce
    sums them over ranks).  relu: is there an activation behind the batch norm (default: `y is not None`).  With one, the relu
    mask is recomputed from z (z * scale + shift > 0 with the scale / shift the forward pass left in `st`) for the trunk's
    channel counts (64 .. 2048, powers of two) -- a third less traffic, and `y` is then NOT read and may be None
    (`relu=True`); other channel counts, and mask_from_z=False, read the mask from y, which must then be given."""
    lib = _lib.lib()
    if ups8_of is not None:     # z = bilinear_x8(ups8_of), recomputed per element (relu behind the batch norm, mask from z)
        _lib.check(lib.xv_bn_bwd_reduce_zmask_ups8(dy.xv(), ups8_of.xv(), _ptr(st.mean), _ptr(st.invstd), _ptr(st.scale),
                                                   _ptr(st.shift), _ptr(st.sums), _ptr(dgamma), _ptr(dbeta), *st.wsp(), _stream()),
                   'xv_bn_bwd_reduce_zmask_ups8')
        mult = _sync_sums(st, sync)
        _lib.check(lib.xv_bn_bwd_apply_zmask_ups8(dy.xv(), ups8_of.xv(), _ptr(st.mean), _ptr(st.invstd), _ptr(st.scale),
                                                  _ptr(st.shift), _ptr(gamma), _ptr(st.sums), dy.n * dy.h * dy.w * mult, dz.xv(),
                                                  _stream()), 'xv_bn_bwd_apply_zmask_ups8')
        return dz
    if relu is None:
        relu = y is not None
    can_zmask = z.c >= 64 and 2048 % z.c == 0
    if mask_from_z is None:
        mask_from_z = relu and can_zmask
    if relu and not mask_from_z and y is None:
        raise ValueError('bn_backward: %d channels take the relu mask from y (none given)' % z.c)
    if not relu:
        y = None
    if mask_from_z and relu:
        _lib.check(lib.xv_bn_bwd_reduce_zmask(dy.xv(), z.xv(), _ptr(st.mean), _ptr(st.invstd), _ptr(st.scale), _ptr(st.shift),
                                              _ptr(st.sums), _ptr(dgamma), _ptr(dbeta), *st.wsp(), _stream()),
                   'xv_bn_bwd_reduce_zmask')
        mult = _sync_sums(st, sync)
        _lib.check(lib.xv_bn_bwd_apply_zmask(dy.xv(), z.xv(), _ptr(st.mean), _ptr(st.invstd), _ptr(st.scale), _ptr(st.shift),
                                             _ptr(gamma), _ptr(st.sums), z.n * z.h * z.w * mult, dz.xv(), _stream()),
                   'xv_bn_bwd_apply_zmask')
        return dz
    yx = y.xv() if y is not None else _NULL_ACT
    _lib.check(lib.xv_bn_bwd_reduce_ws(dy.xv(), yx, z.xv(), _ptr(st.mean), _ptr(st.invstd), _ptr(st.sums), _ptr(dgamma),
                                       _ptr(dbeta), *st.wsp(), _stream()), 'xv_bn_bwd_reduce_ws')
    mult = _sync_sums(st, sync)
    _lib.check(lib.xv_bn_bwd_apply(dy.xv(), yx, z.xv(), _ptr(st.mean), _ptr(st.invstd), _ptr(gamma), _ptr(st.sums),
                                   z.n * z.h * z.w * mult, dz.xv(), _stream()), 'xv_bn_bwd_apply')
    return dz


def bn_pool_backward(dpooled, z, gamma, st, dgamma, dbeta, dz, sync=False):
    """dz of a conv -> batch norm -> relu -> 2x2 max-pool block from the gradient of the POOLED map: MaxPoolGrad, ReluGrad
    and the batch-norm gradient in the two normalisation passes (the routed full-resolution gradient never reaches HBM)."""
    lib = _lib.lib()
    _lib.check(lib.xv_bn_pool_bwd_reduce(dpooled.xv(), z.xv(), _ptr(st.mean), _ptr(st.invstd), _ptr(st.scale), _ptr(st.shift),
                                         _ptr(st.sums), _ptr(dgamma), _ptr(dbeta), *st.wsp(), _stream()), 'xv_bn_pool_bwd_reduce')
    mult = _sync_sums(st, sync)
    _lib.check(lib.xv_bn_pool_bwd_apply(dpooled.xv(), z.xv(), _ptr(st.mean), _ptr(st.invstd), _ptr(st.scale), _ptr(st.shift),
                                        _ptr(gamma), _ptr(st.sums), z.n * z.h * z.w * mult, dz.xv(), _stream()),
               'xv_bn_pool_bwd_apply')
    return dz


def bn_dense_forward(z, gamma, beta, moving_mean, moving_var, st, y, sync=False):
    """The same on a dense float32 [..., C] tensor (no activation)."""
    lib = _lib.lib()
    c = z.shape[-1]
    rows = z.numel() // c
    _lib.check(lib.xv_bn_dense_stats_ws(_ptr(z), rows, c, _ptr(st.sums), *st.wsp(), _stream()), 'xv_bn_dense_stats_ws')
    mult = _sync_sums(st, sync)
    _lib.check(lib.xv_bn_finalize(_ptr(st.sums), c, rows * mult, _ptr(gamma), _ptr(beta), BN_EPS, BN_MOMENTUM,
                                  _ptr(moving_mean), _ptr(moving_var), _ptr(st.mean), _ptr(st.invstd), _ptr(st.scale),
                                  _ptr(st.shift), _stream()), 'xv_bn_finalize')
    if y is not None:       # (y = None: the caller applies st.scale / st.shift itself, e.g. softmax_ce_dense(affine=st))
        _lib.check(lib.xv_bn_dense_apply(_ptr(z), rows, c, _ptr(st.scale), _ptr(st.shift), _ptr(y), _stream()),
                   'xv_bn_dense_apply')
    return y


def bn_dense_backward(dy, z, gamma, st, dgamma, dbeta, dz, sync=False):
    lib = _lib.lib()
    c = z.shape[-1]
    rows = z.numel() // c
    _lib.check(lib.xv_bn_dense_bwd_reduce_ws(_ptr(dy), _ptr(z), rows, c, _ptr(st.mean), _ptr(st.invstd), _ptr(st.sums),
                                             _ptr(dgamma), _ptr(dbeta), *st.wsp(), _stream()), 'xv_bn_dense_bwd_reduce_ws')
    mult = _sync_sums(st, sync)
    _lib.check(lib.xv_bn_dense_bwd_apply(_ptr(dy), _ptr(z), rows, c, _ptr(st.mean), _ptr(st.invstd), _ptr(gamma),
                                         _ptr(st.sums), rows * mult, _ptr(dz), _stream()), 'xv_bn_dense_bwd_apply')
    return dz


def upsample_raw_fwd(x, factor, y=None):
    if y is None:
        y = Act(x.n, factor * x.h, factor * x.w, x.c, x.t.device)
    _lib.check(_lib.lib().xv_upsample_raw_fwd(x.xv(), factor, y.xv(), _stream()), 'xv_upsample_raw_fwd')
    return y


_UPS_WS = {}
UPS8_BLOCK_SUMS = True      # False (a test seam): the gather form of the x8 gradient


def upsample_raw_bwd(dy, factor, dx):
    """Gradient of the raw bilinear up-sampling.  factor 8: through per-block sums in a workspace (one per device and stream,
    grown to the largest map seen), every element of dy read once."""
    lib = _lib.lib()
    if factor == 8 and UPS8_BLOCK_SUMS:
        key = (dx.t.device, _stream().value)
        need = max(16, lib.xv_upsample_raw_bwd_workspace_bytes(dx.n, dx.h, dx.w, dx.c)) // 4
        ws = _UPS_WS.get(key)
        if ws is None or ws.numel() < need:
            ws = _UPS_WS[key] = torch.empty(need, dtype=torch.float32, device=dx.t.device)
        _lib.check(lib.xv_upsample_raw_bwd_ws(dy.xv(), factor, dx.xv(), _ptr(ws), ws.numel() * 4, _stream()), 'xv_upsample_raw_bwd_ws')
        return dx
    _lib.check(lib.xv_upsample_raw_bwd(dy.xv(), factor, dx.xv(), _stream()), 'xv_upsample_raw_bwd')
    return dx


def bn_apply_ups8(low, st, y, relu=True):
    """y = [relu](bilinear_x8(low) * scale + shift) with the scale / shift bn_forward(ups8_of=low, y=None) left in `st`."""
    _lib.check(_lib.lib().xv_bn_apply_ups8(low.xv(), _ptr(st.scale), _ptr(st.shift), int(bool(relu)), y.xv(), _stream()),
               'xv_bn_apply_ups8')
    return y


def score_dense_fwd_ups8(low, st, w_score, b_score, num_classes, y, score):
    """y = relu(BN(bilinear_x8(low))) with the batch norm's scale / shift in `st` (bn_forward(ups8_of=low, y=None) before this)
    AND score = y . W + b in one launch.  Returns False -- nothing launched -- where the fused kernel does not take the shape."""
    rc = _lib.lib().xv_score_dense_fwd_ups8(low.xv(), _ptr(st.scale), _ptr(st.shift), _ptr(w_score), _ptr(b_score), num_classes,
                                            y.xv(), _ptr(score), _stream())
    if rc == XV_ESHAPE:
        return False
    _lib.check(rc, 'xv_score_dense_fwd_ups8')
    return True


def score_dense_fwd(u, w_score, b_score, num_classes, score):
    _lib.check(_lib.lib().xv_score_dense_fwd(u.xv(), _ptr(w_score), _ptr(b_score), num_classes, _ptr(score), _stream()),
               'xv_score_dense_fwd')
    return score


_CE_WS = {}


def softmax_ce_dense(logits, labels, count, num_classes, loss, dlogits, affine=None):
    """affine (a BnState): `logits` holds raw scores, logits = scores * affine.scale + affine.shift inside the kernel.
    The loss is added up in a fixed order (xv_softmax_ce_dense_ws: per-workgroup partials in a workspace kept per device and
    stream, one small launch adds them): bitwise reproducible, like the rest of the training step."""
    _need(labels, torch.int32, 'labels')
    npix = labels.numel()
    key = (logits.device, _stream().value)
    nbytes = _lib.lib().xv_softmax_ce_dense_workspace_bytes(npix)
    ws = _CE_WS.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _CE_WS[key] = torch.empty(max(nbytes // 8, 2048), dtype=torch.float64, device=logits.device)
    _lib.check(_lib.lib().xv_softmax_ce_dense_ws(_ptr(logits), _ptr(affine.scale) if affine is not None else None,
                                                 _ptr(affine.shift) if affine is not None else None, _ptr(labels),
                                                 _ptr(count), num_classes, npix, _ptr(loss), _ptr(dlogits), _ptr(ws),
                                                 ws.numel() * 8, _stream()), 'xv_softmax_ce_dense_ws')
    return dlogits


_SD_WS = {}


def score_dense_bwd(u, dscore, w_score, num_classes, dw_score, db_score, du):
    """Backward of the dense 1x1 score layer at full resolution; filter and bias gradients added in a fixed order (a workspace
    per device and stream, grown to the largest map seen): bitwise reproducible."""
    lib = _lib.lib()
    key = (u.t.device, _stream().value)
    need = max(16, lib.xv_score_dense_bwd_workspace_bytes(u.n, u.h, u.w)) // 4
    ws = _SD_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _SD_WS[key] = torch.empty(need, dtype=torch.float32, device=u.t.device)
    rc = lib.xv_score_dense_bwd_ws(u.xv(), _ptr(dscore), _ptr(w_score), num_classes, _ptr(dw_score), _ptr(db_score), du.xv(),
                                   _ptr(ws), ws.numel() * 4, _stream())
    _lib.check(rc, 'xv_score_dense_bwd_ws')
    return du


# ---- on-device training augmentation (csrc/augment.hip) ----------------------------------------------------------------------

def augment_plan_bytes():
    return int(_lib.lib().xv_augment_plan_bytes())


def augment_batch(pool, index, plans, luts):
    """The host augmentation chain for a batch in one launch (include/xview_hip.h xv_augment_batch).

    pool    {'rgb': uint8 [M,H,W,3], 'depth': uint16 [M,H,W] or [M,H,W,1], 'labels': int32 [M,H,W]} resident tensors
    index   host int32 [N]: the source image of each output image
    plans   host numpy record array [N] of xv_augment_plan (datasets/device_augmentation.py pack_plans)
    luts    host uint8 [N,256]: the composed photometric table of each output image
    Index, plans and tables travel to the device in ONE copy; the call checks its host copies of them and refuses
    (XvError: XV_EINVAL) before anything is launched.  Returns rgb float32 [N,S,S,3], depth float32 [N,S,S,1], labels int32
    [N,S,S] with S the plans' crop size cut down to a multiple of 16."""
    import numpy as np
    rgb, depth, labels = pool['rgb'], pool['depth'], pool['labels']
    _need(rgb, torch.uint8, "pool['rgb']")
    _need(depth, torch.uint16, "pool['depth']")
    _need(labels, torch.int32, "pool['labels']")
    M, H, W = rgb.shape[:3]
    if tuple(rgb.shape) != (M, H, W, 3) or tuple(depth.shape) not in ((M, H, W), (M, H, W, 1)) or \
            tuple(labels.shape) != (M, H, W):
        raise ValueError('pool shapes %s / %s / %s are not [M,H,W,3] / [M,H,W(,1)] / [M,H,W] of one size' % (
            tuple(rgb.shape), tuple(depth.shape), tuple(labels.shape)))
    index = np.ascontiguousarray(index, dtype=np.int32)
    plans = np.ascontiguousarray(plans)
    luts = np.ascontiguousarray(luts, dtype=np.uint8)
    N = len(index)
    if plans.dtype.itemsize != augment_plan_bytes():
        raise ValueError('plan records of %d bytes, the library takes %d' % (plans.dtype.itemsize, augment_plan_bytes()))
    if N < 1 or plans.shape != (N,) or luts.shape != (N, 256):
        raise ValueError('index [N], plans [N] and luts [N,256] must agree (N >= 1)')
    sizes = set(int(s) for s in plans['crop_size'])
    if len(sizes) != 1:
        raise ValueError('the plans of one batch crop to different sizes: %s' % sorted(sizes))
    S = sizes.pop() // 16 * 16
    # one host buffer, one upload: records (8-byte aligned at the front), then the indices, then the tables
    host = np.concatenate([plans.view(np.uint8).reshape(-1), index.view(np.uint8), luts.reshape(-1)])
    dev = torch.from_numpy(host).to(rgb.device)
    nplan, nidx = plans.nbytes, index.nbytes
    out_rgb = torch.empty((N, max(S, 0), max(S, 0), 3), dtype=torch.float32, device=rgb.device)
    out_depth = torch.empty((N, max(S, 0), max(S, 0), 1), dtype=torch.float32, device=rgb.device)
    out_labels = torch.empty((N, max(S, 0), max(S, 0)), dtype=torch.int32, device=rgb.device)
    base = dev.data_ptr()
    rc = _lib.lib().xv_augment_batch(_ptr(rgb), _ptr(depth), _ptr(labels), M, H, W, ctypes.c_void_p(base + nplan),
                                     index.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(base),
                                     plans.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(base + nplan + nidx), N, S,
                                     _ptr(out_rgb), _ptr(out_depth), _ptr(out_labels), _stream())
    _lib.check(rc, 'xv_augment_batch')
    return out_rgb, out_depth, out_labels
