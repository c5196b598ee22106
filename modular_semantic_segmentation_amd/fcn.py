"""The FCN expert on MI355X: host-side mirror of `encoder` / `decoder` / `fcn`
(xview/models/simple_fcn.py:10-170) driving the HIP kernels through the C ABI.

Data layout in HBM: bf16 padded-NHWC activations (see ops.Act), packed bf16 conv weights,
fp32 first-layer / score weights.  Per image and stream the encoder runs 13 convs (12 on MFMA;
pool1..pool4 fused into the epilogues of conv1_2/2_2/3_3/4_3), two 1x1 score convs, the x2
bilinear + add, and ONE fused decoder-head kernel (x8 bilinear + relu + score + softmax + argmax).
"""
import numpy as np
import torch

from . import ops
from .custom_layers import bilinear_filter, dense_deconv_as_conv3x3, is_bilinear_filter

ENCODER = [  # (name, cout, pool_after)   simple_fcn.py:39-67
    ('conv1_1', 64, None), ('conv1_2', 64, 'pool1'),
    ('conv2_1', 128, None), ('conv2_2', 128, 'pool2'),
    ('conv3_1', 256, None), ('conv3_2', 256, None), ('conv3_3', 256, 'pool3'),
    ('conv4_1', 512, None), ('conv4_2', 512, None), ('conv4_3', 512, 'pool4'),
    ('conv5_1', 512, None), ('conv5_2', 512, None), ('conv5_3', 512, None)]
BN_EPS = 1e-3  # [TF1] tf.layers.batch_normalization default epsilon
# conv_dtype='fp8' (BASELINE config "fp8 MFMA conv path"): the convs from 128 input channels up run on the block-scaled
# e4m3 MFMA kernels; conv1_1 reads the raw fp32 input; the two 1x1 score convs read fp8 and write bf16 for the fp32
# decoder head.  conv2_1 (64 input channels) is an e4m3 conv on the generation-4 kernel, conv1_2 only with fp8_deep: see
# fp8_plan().
FP8_CONVS = ('conv2_2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv4_1', 'conv4_2', 'conv4_3', 'conv5_1', 'conv5_2', 'conv5_3')
# conv outputs that may be stored as e4m3, each with a calibrated scale (pools inherit their conv's scale)
FP8_MAPS = ('conv1_1', 'conv1_2', 'conv2_1') + FP8_CONVS


# how calibrate() chooses an activation map's exponent unless told otherwise: 'max' (largest magnitude + one bit of headroom);
# calibrate(method='mse') takes the least squared e4m3 error on the calibration batch
FP8_CALIBRATION = 'max'
FP8_DEFAULT_START = 'conv2_2'
# the accuracy-guarded plan (FcnEngine.calibrate_guarded): first e4m3 conv candidates from the deepest plan (most layers on
# e4m3 operands) to the shallowest; an expert that fails the bound on all of them runs on bf16 operands
FP8_GUARD_CANDIDATES = ('conv2_2', 'conv3_1', 'conv4_1', 'conv5_1')
FP8_GUARD_AGREEMENT = 0.995


def padded_units(num_units):
    """Lanes the `num_units`-channel decoder maps are padded to (zero weights, zero maps): 64, 128 or 256 -- the widths every
    kernel behind them takes, the batch-norm passes of training included (batchnorm.hip: C >= 64, 2048 % C == 0; a 192-lane
    map has no statistics kernel) -- and multiples of 64 beyond 256 (inference; the batch-norm trainers refuse those)."""
    u = int(num_units)
    for lanes in (64, 128, 256):
        if u <= lanes:
            return lanes
    return (u + 63) // 64 * 64


def fp8_plan(h=None, w=None, deep=False, start=None):
    """(convs with e4m3 operands, conv outputs stored as e4m3) of conv_dtype='fp8': the convs from `start` on take e4m3
    operands, the conv in front of `start` is a bf16 conv that writes the first e4m3 map.

      start='conv2_2' (default since round 5): conv1_1 fp32, conv1_2 and conv2_1 bf16, conv2_1 writes the first e4m3 map.
          tools/fp8_calib_study.py on trained experts: the depth expert (classes are thresholds on ONE raw uint16 channel, so
          its first pooled map carries the information in small relative differences) loses 2.9 - 3.7 points of mIoU when
          pool1 is stored with 3-bit mantissas and 0.01 when the first e4m3 map is conv2_1's; the RGB expert is within 0.06
          either way.  conv2_1 is 6 % of the FLOPs: ~3 % of the step at 2048x1024.
      start='conv2_1' (model config `fp8_start`; the default of rounds 2-4): conv1_2 writes the first e4m3 map (pool1).
      deep=True (model config `fp8_deep`) = start='conv1_2': conv1_1 writes the first e4m3 map: +14 % images/s at 2048x1024,
          depth expert -6.5 points.
    Any later layer up to conv5_1 may be named as well (the 1x1 score convs read conv4_3 / conv5_3 with e4m3-packed weights:
    a plan that leaves either map in bf16 would hand bf16 operands to those weights).  oracle/fcn_oracle.py states the same
    rule.  (h, w: unused since the kernels handle partial tiles; kept for callers.)"""
    names = [n for n, _, _ in ENCODER]
    start = start or ('conv1_2' if deep else FP8_DEFAULT_START)
    allowed = names[1:names.index('conv5_1') + 1]
    if start not in allowed:
        raise ValueError('fp8_start must be one of %s' % allowed)
    i = names.index(start)
    return tuple(names[i:]), tuple(names[i - 1:])


def variable_shapes(prefix, in_channels, num_units, num_classes, batch_normalization=False):
    """name -> shape of every variable of one FCN expert, in the reference npz schema
    (names: 'Synthia Rand Cityscapes Examples.ipynb':897-931; BN adds gamma/beta/moving_*)."""
    shapes = {}
    cin = in_channels
    for name, cout, _ in ENCODER:
        shapes['%s/%s/kernel' % (prefix, name)] = (3, 3, cin, cout)
        shapes['%s/%s/bias' % (prefix, name)] = (cout,)
        cin = cout
    for name in ('score_conv4', 'score_conv5'):
        shapes['%s/%s/kernel' % (prefix, name)] = (1, 1, 512, num_units)
        shapes['%s/%s/bias' % (prefix, name)] = (num_units,)
    shapes['%s/upscore_conv5/kernel' % prefix] = (4, 4, num_units, num_units)
    shapes['%s/upscore/kernel' % prefix] = (16, 16, num_units, num_units)
    shapes['%s/score/kernel' % prefix] = (1, 1, num_units, num_classes)
    shapes['%s/score/bias' % prefix] = (num_classes,)
    if batch_normalization:
        for key in list(shapes):
            if key.endswith('/kernel'):
                layer = key[:-len('/kernel')]
                c = shapes[key][2] if 'upscore' in layer else shapes[key][3]
                for v in ('gamma', 'beta', 'moving_mean', 'moving_variance'):
                    shapes['%s/%s' % (layer, v)] = (c,)
    return shapes


def init_variables(prefix, in_channels, num_units, num_classes, batch_normalization=False, seed=None):
    """[TF1] default initialisers: Glorot-uniform kernels, zero biases, bilinear deconv constants,
    BN gamma=1 beta=0 mean=0 var=1."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in variable_shapes(prefix, in_channels, num_units, num_classes, batch_normalization).items():
        leaf = name.rsplit('/', 1)[1]
        if 'upscore' in name and leaf == 'kernel':
            out[name] = bilinear_filter(shape)
        elif leaf == 'kernel':
            kh, kw, cin, cout = shape
            lim = np.sqrt(6.0 / (kh * kw * cin + kh * kw * cout))
            out[name] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
        elif leaf in ('gamma', 'moving_variance'):
            out[name] = np.ones(shape, np.float32)
        else:
            out[name] = np.zeros(shape, np.float32)
    return out


def _fold_bn(variables, layer, kernel, bias):
    """Inference batch-norm after the conv (custom_layers.py:126-137, BN before the activation):
    y = gamma*(conv+b-mean)/sqrt(var+eps)+beta  ==  conv(x, W*s) + ((b-mean)*s+beta)."""
    g = variables.get(layer + '/gamma')
    if g is None:
        return kernel, bias
    s = g / np.sqrt(variables[layer + '/moving_variance'] + BN_EPS)
    return kernel * s, (bias - variables[layer + '/moving_mean']) * s + variables[layer + '/beta']


def check_variables(v, shapes):
    """Every variable of `shapes` (name -> shape) is in the dict `v`, with that shape."""
    for need, shape in shapes.items():
        if need not in v:
            raise KeyError('missing variable %s' % need)
        if tuple(np.shape(v[need])) != tuple(shape):
            raise ValueError('variable %s has shape %s, expected %s' % (need, np.shape(v[need]), shape))


def upload(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


# ---- the decoder tail of FcnEngine and fusion_fcn.FusionFcnEngine: weights --------------------------------------------------
def dense_deconv_weights(kern, stride, U, Up, device):
    """The reference never trains its deconvs (simple_fcn.py:80-83,117-119; fusion_fcn.py:26-31), so their kernels are the
    bilinear constant and run as depthwise interpolations: None.  An imported kernel that is anything else takes the dense
    transposed-conv path (xv_deconv_dense_fwd on the MFMA conv; the decoder head is then the un-commuted one): its 3x3 phase
    weights, padded to Up units and packed, and their zero bias."""
    if is_bilinear_filter(kern):
        return None
    kp = np.zeros((kern.shape[0], kern.shape[1], Up, Up), np.float32)
    kp[:, :, :U, :U] = kern                                 # padding units: zero rows and columns
    k3 = torch.from_numpy(dense_deconv_as_conv3x3(kp, stride)).to(device)
    return ops.pack_conv_weights(k3), torch.zeros(stride * stride * Up, dtype=torch.float32, device=device)


def deconv_batch_norm(v, layer, U, Up, device, dense):
    """Batch norm after a deconv (custom_layers.py:112-119) is a per-channel affine before its relu: (scale, affine).  A
    positive scale with zero shift commutes with the relu and the (linear, bilinear: not `dense`) deconv: `scale`, for the
    caller to fold into the 1x1 conv on the other side.  Anything else goes through the affine forms of the x2 kernel and of
    the decoder head (the un-commuted one: 16x the FMAs of the default head): `affine`, padded to Up.  No batch norm: neither."""
    if layer + '/gamma' not in v:
        return None, None
    s = v[layer + '/gamma'] / np.sqrt(v[layer + '/moving_variance'] + BN_EPS)
    t = v[layer + '/beta'] - v[layer + '/moving_mean'] * s
    if np.all(s > 0) and np.all(np.abs(t) <= 1e-12) and not dense:
        return s.astype(np.float32), None
    sp, tp = np.ones(Up, np.float32), np.zeros(Up, np.float32)
    sp[:U], tp[:U] = s, t                                   # padding channels: relu(0 * 1 + 0) = 0
    return None, (upload(sp, device), upload(tp, device))


def padded_score_conv(k, b, U, Up):
    """A 1x1 score conv [1,1,cin,U] (cin: 512 per trunk) padded to Up lanes of zeros: the score convs run on the MFMA kernel."""
    kp = np.zeros((1, 1, k.shape[2], Up), np.float32)
    kp[..., :U] = k
    bp = np.zeros(Up, np.float32)
    bp[:U] = b
    return kp, bp


def padded_score_matrix(k, Up, device):
    """The class-score matrix [U,C] of the decoder head with zero rows for the padding units, on the device."""
    ws = np.zeros((Up, k.shape[1]), np.float32)
    ws[:k.shape[0]] = k
    return upload(ws, device)


# ---- the decoder tail: launches (e: the engine -- _act, _arena, Up, C, w['score'], b['score']) -------------------------------
def upsample2x_skip(e, s5, s4, y, dense, affine):
    """y = relu(x2 deconv of s5 [batch norm `affine`]) + s4; dense: dense_deconv_weights of the deconv kernel"""
    scale, shift = affine or (None, None)
    if dense is not None:
        wk, zb = dense
        _, e._arena['dd_ws5'] = ops.deconv_dense_fwd(s5, wk, zb, 2, e.Up, y=y, scale=scale, shift=shift, residual=s4, relu=True,
                                                    workspace=e._arena.get('dd_ws5'))
    else:
        ops.upsample2x_relu_add(s5, residual=s4, y=y, scale=scale, shift=shift)
    return y


def decoder_head(e, f, want, dense, affine, layers, workspace=None):
    """The head, from the decoder's input `f` to a dict with the wanted 'score' / 'prob' (float32 [N,H,W,C]) / 'label' (int64
    [N,H,W]): ONE kernel, or with a `dense` x8 deconv kernel the dense deconv -> [batch norm] -> relu at full resolution
    (layers['upscore']), then the per-pixel score conv, softmax, argmax."""
    scale, shift = affine or (None, None)
    want_label = 'label' in want or 'classification' in want
    if dense is None:
        return ops.decoder_head_fwd(f, e.w['score'], e.b['score'], e.C, want_score='score' in want, want_prob='prob' in want,
                                    want_label=want_label, workspace=workspace, scale=scale, shift=shift)
    wk, zb = dense
    up = layers['upscore'] = e._act('upscore', f.n, 8 * f.h, 8 * f.w, e.Up)
    _, e._arena['dd_ws'] = ops.deconv_dense_fwd(f, wk, zb, 8, e.Up, y=up, scale=scale, shift=shift, relu=True,
                                               workspace=e._arena.get('dd_ws'))
    skey = ('dense_score', f.n, f.h, f.w)
    if skey not in e._arena:
        e._arena[skey] = torch.empty((f.n, 8 * f.h, 8 * f.w, e.C), dtype=torch.float32, device=e.device)
    score = ops.score_dense_fwd(up, e.w['score'], e.b['score'], e.C, e._arena[skey])
    prob, label = ops.softmax_argmax(score, want_prob='prob' in want, want_label=want_label)
    out = {'score': score} if 'score' in want else {}
    if prob is not None:
        out['prob'] = prob
    if label is not None:
        out['label'] = label
    return out


# The two experts of a fusion model run the same layer shapes from conv1_2 on.  From this layer on each 3x3 layer of both is
# ONE launch (ops.conv2d_fwd_pair: whole rounds of workgroups where each expert alone leaves its last round half empty).
# (A test seam: another layer name moves the start, a name that is no layer keeps every launch per expert -- same bits.)
GROUP_FROM = 'conv4_1'


def group_from_index():
    names = [e[0] for e in ENCODER]
    return names.index(GROUP_FROM) if GROUP_FROM in names else None


def encoder_layers_pair(ea, sa, eb, sb):
    """The remaining encoder layers of two engines (states from encoder_begin(..., stop=group_from_index())), each layer as
    one launch for both where the kernel takes the shape, else one launch per engine."""
    assert sa['next'] == sb['next']
    for idx in range(sa['next'], len(ENCODER)):
        name = ENCODER[idx][0]
        ya, qa = ea._layer_outputs(sa, idx)
        yb, qb = eb._layer_outputs(sb, idx)
        if not ops.conv2d_fwd_pair(sa['cur'], ea.w[name], ea.b[name], sb['cur'], eb.w[name], eb.b[name], relu=True,
                                   ya=ya, yb=yb, pa=qa, pb=qb):
            for e, st, y, q in ((ea, sa, ya, qa), (eb, sb, yb, qb)):
                ops.conv2d_fwd(st['cur'], e.w[name], e.b[name], 3, relu=True, y=y, pooled=q, write_y=y is not None)
        ea._layer_done(sa, idx, ya, qa)
        eb._layer_done(sb, idx, yb, qb)


class Arena(object):
    """An engine's device buffers, kept from call to call in the plain dict `self._arena` (on `self.device`): activations by
    name, shape and dtype; route buffers and workspaces under keys of their own."""

    def _act(self, name, n, h, w, c, dtype='bf16', scale_exp=0):
        key = (name, n, h, w, c, dtype)
        a = self._arena.get(key)
        if a is None:
            a = ops.Act(n, h, w, c, self.device, dtype=dtype, scale_exp=scale_exp)
            self._arena[key] = a
        elif a.scale_exp != scale_exp:
            a.set_scale_exp(scale_exp)
        return a


class Vgg16Walk(Arena):
    """The 13 convs of ENCODER (pool1..pool4 fused into the conv epilogues) over a host object with `cin`, the weights `w` /
    `b` by layer name and an arena: the ONLY walk of the trunk -- the FCN expert in bf16 and fp8, alone or paired with a twin
    (encoder_layers_pair), and the trunks of the joint model (fusion_fcn.VggTrunk).  In steps over a state dict, so that a
    fusion model can pair launches and the MC-dropout samplers can resume a state: encoder_begin (input checks, the first
    conv(s), the layers before `stop`), then encoder_layers.  What differs between the callers are these options:"""
    streamk = False         # hand the 3x3 convs of a bf16 walk a stream-K workspace (_sk)
    split_small = False     # un-pooled layers of a bf16 walk: the split form where the tiles fill less than half the CUs

    def _drop_fn(self):
        """The dropout sites of the walk: a function (Act, tag) -> dropped Act, or None"""
        return None

    def _fp8_plan(self, x):
        """(convs with e4m3 operands, conv outputs stored as e4m3) of a walk over x: see fp8_plan(); ((), ()) is bf16"""
        return (), ()

    def _sk(self):
        """This engine's stream-K workspace (ops.streamk_workspace: arrival counters + partial-tile slabs of the
        generation-2 conv kernel's tail round).  One per engine: the two experts of a fusion model run on two streams."""
        if not self.streamk:
            return None
        ws = self._arena.get('streamk_ws')
        if ws is None:
            ws = self._arena['streamk_ws'] = ops.streamk_workspace(self.device)
        return ws

    def _state(self, n, h, w, cur=None, next=0, keep_all=False, routed=False, plan=((), ())):
        """The state of a walk over n images of h x w that has come to layer `next` with the map `cur`"""
        return {'n': n, 'h': h, 'w': w, 'keep_all': keep_all, 'routed': routed, 'convs8': plan[0], 'maps8': plan[1], 'L': {},
                'cur': cur, 'ch': cur.h if cur is not None else h, 'cw': cur.w if cur is not None else w, 'next': next}

    def _weights(self, st, name):
        return self.w8[name] if name in st['convs8'] else self.w[name]

    def _stored(self, st, name):
        """dtype / scale_exp of the maps conv `name` writes (a pool inherits its conv's scale), as _act arguments"""
        return dict(dtype='fp8', scale_exp=self.fp8_scales[name]) if name in st['maps8'] else {}

    def encoder_begin(self, x, keep_all=False, stop=None, routed=False):
        n, h, w, cin = x.shape
        if cin != self.cin:
            raise ValueError('expected %d input channels, got %d' % (self.cin, cin))
        if h % 16 or w % 16:
            raise ValueError('H and W must be multiples of 16 (augmentation.py:244-262 crop_multiple)')
        plan = convs8, maps8 = self._fp8_plan(x)
        # route bytes: the training step's (keep_all) bf16 walk only
        st = self._state(n, h, w, keep_all=keep_all, routed=bool(routed) and keep_all and not maps8, plan=plan)
        x = x.contiguous()
        # conv1_1 + conv1_2 + pool1 in one launch where neither full-resolution map is wanted (inference): conv1_1 is
        # evaluated straight into conv1_2's LDS patch buffers (csrc/conv_first_fused.hip; the same bits as the two kernels,
        # also in its e4m3-out form).  Maps that do not tile in 16x32 take the two kernels, and so does an fp8 plan that stores
        # conv1_1 as e4m3 or gives conv1_2 e4m3 operands.  (fp8_start behind conv2_1: pool1 stays bf16.)
        if not keep_all and 'conv1_1' not in maps8 and 'conv1_2' not in convs8 and \
                ENCODER[1][0] == 'conv1_2' and ENCODER[1][2] == 'pool1':
            q = self._act('pool1', n, h // 2, w // 2, 64, **self._stored(st, 'conv1_2'))
            if ops.conv_first_pair_fwd(x, self.w['conv1_1'], self.b['conv1_1'], self.w['conv1_2'], self.b['conv1_2'], pooled=q):
                st['L']['pool1'] = st['cur'] = q
                st.update(ch=h // 2, cw=w // 2, next=2)
        if st['next'] == 0:
            y = self._act('conv1_1', n, h, w, 64, **self._stored(st, 'conv1_1'))
            ops.conv2d_first_fwd(x, self.w['conv1_1'], self.b['conv1_1'], y, relu=True)
            st['L']['conv1_1'] = st['cur'] = y
            st['next'] = 1
        self.encoder_layers(st, len(ENCODER) if stop is None else stop)
        return st

    def _layer_outputs(self, st, idx):
        """(full map or None, pooled map or None) of encoder layer idx"""
        name, cout, pool = ENCODER[idx]
        n, ch, cw, kw = st['n'], st['ch'], st['cw'], self._stored(st, name)
        if pool is None:
            return self._act(name, n, ch, cw, cout, **kw), None
        need_full = st['keep_all'] or name == 'conv4_3'       # conv4_3 feeds score_conv4
        return (self._act(name, n, ch, cw, cout, **kw) if need_full else None), self._act(pool, n, ch // 2, cw // 2, cout, **kw)

    def _layer_done(self, st, idx, y, q):
        name, cout, pool = ENCODER[idx]
        L = st['L']
        if pool is None:
            L[name] = st['cur'] = y
        else:
            if y is not None:
                L[name] = y
            L[pool] = st['cur'] = q
            st['ch'], st['cw'] = st['ch'] // 2, st['cw'] // 2
            # simple_fcn.py:51-63: the dropout after pool4 is gated by 'pool3' too (a quirk of the reference:
            # 'pool4' alone enables nothing)
            drop = self._drop_fn()
            if drop is not None and pool in ('pool3', 'pool4') and 'pool3' in self.dropout_layers:
                L[pool + '_drop'] = st['cur'] = drop(q, pool + '_drop')
        st['next'] = idx + 1

    def encoder_layers(self, st, stop):
        """encoder layers [st['next'], stop), one launch each"""
        bf16 = not st['maps8']
        for idx in range(st['next'], stop):
            name = ENCODER[idx][0]
            y, q = self._layer_outputs(st, idx)
            # routed: a conv in front of a pool whose full map only MaxPoolGrad would read leaves the pool's route bytes instead
            # (never conv4_3: it feeds score_conv4)
            if st['routed'] and q is not None and name != 'conv4_3' and self._drop_fn() is None:
                key = ('route_' + name, st['n'], q.h, q.w, q.c)
                route = self._arena.get(key)
                if route is None:
                    route = self._arena[key] = torch.empty(st['n'] * q.h * q.w * q.c, dtype=torch.uint8, device=self.device)
                if ops.conv2d_fwd_route(st['cur'], self.w[name], self.b[name], q, route):
                    st['L']['route_' + name] = route
                    self._layer_done(st, idx, None, q)
                    continue
            split = self.split_small and bf16 and q is None
            ops.conv2d_fwd(st['cur'], self._weights(st, name), self.b[name], 3, relu=True, y=y, pooled=q, write_y=y is not None,
                           workspace=self._sk() if bf16 else None,
                           split_ws=ops.split_workspace(st['cur'], ENCODER[idx][1], self._arena) if split else None)
            self._layer_done(st, idx, y, q)


class FcnEngine(Vgg16Walk):
    """One FCN expert resident on one GPU (inference graph of simple_fcn.py:137-170)."""
    split_small = True

    def __init__(self, prefix, in_channels, num_units, num_classes, variables, device='cuda', conv_dtype='bf16',
                 streamk=False, fp8_deep=False, fp8_start=None):
        self.prefix, self.cin, self.U, self.C = prefix, int(in_channels), int(num_units), int(num_classes)
        self.device = torch.device(device)
        self.Up = padded_units(self.U)            # score convs run on the MFMA kernel: pad U to 64 / 128 / 256 / ... lanes of zeros
        if conv_dtype not in ('bf16', 'fp8'):
            raise ValueError("conv_dtype must be 'bf16' or 'fp8'")
        self.conv_dtype = conv_dtype
        # streamk: hand the 3x3 convs a stream-K workspace (ops.streamk_workspace) -- the kernel then splits the tiles of an
        # incomplete last round over idle CUs where that pays (conv5_x at one image: 46 -> 27 us).  Off by default: which
        # tiles are split depends on the batch size, so an image's logits would no longer be bit-identical alone and in a
        # batch (different fp32 groupings; still bitwise reproducible run to run).  A latency option for batch 1.
        self.streamk = bool(streamk)
        self.fp8_deep = bool(fp8_deep)          # conv_dtype='fp8': e4m3 operands from conv1_2 on (see fp8_plan)
        # conv_dtype='fp8': the first conv with e4m3 operands (fp8_plan); a dict {prefix or modality: layer} picks per expert
        if isinstance(fp8_start, dict):
            fp8_start = fp8_start.get(prefix)
        # fp8_start='bf16': this expert of an fp8 model keeps bf16 operands throughout (what calibrate_guarded falls back to)
        self.fp8_off = fp8_start == 'bf16'
        self.fp8_start = None if self.fp8_off else fp8_start
        self.fp8_guard = None                     # report of the last calibrate_guarded()
        self.fp8_scales = None                    # {map name: power-of-two exponent}, set by calibrate()
        # MC dropout (simple_fcn.py:50-62,71-78,124-126; only the uncertainty models enable it): sites after which
        # tf.layers.dropout(training=True) is applied -- 'pool3', 'conv4_3', 'conv5_3' in the encoder, 'features' for the
        # decoder input -- at rate dropout_rate; every forward pass draws new masks (dropout_seed + pass counter)
        self.dropout_layers, self.dropout_rate, self.dropout_seed, self._dropout_pass = (), 0.0, 0, 0
        # mc_lowres_scores: most images one launch of the replicated part of the trunk sees (the samples run in chunks)
        self.mc_chunk_images = 64
        self._arena = {}
        self.load(variables)

    # ---- weights -----------------------------------------------------------------------------
    def load(self, variables):
        p, dev = self.prefix, self.device
        # new weights -> new activation ranges: the fp8 exponents of the previous weights would saturate (or underflow)
        # silently, so the next batch seen calibrates again (or the caller calls calibrate()).  An EXPLICIT calibration is not
        # dropped silently: the first batch after this would become the calibration set (a host sync, and exponents that
        # depend on which batch comes first -- per rank under data parallelism).
        if getattr(self, 'fp8_scales', None) is not None and getattr(self, '_fp8_explicit', False):
            import warnings
            warnings.warn('FcnEngine.load(): new weights invalidate the fp8 calibration of %r; call calibrate() again '
                          '(otherwise the next batch seen is used)' % self.prefix, RuntimeWarning, stacklevel=2)
        self.fp8_scales, self._fp8_explicit = None, False
        if getattr(self, 'fp8_guard', None) is not None:
            # a plan calibrate_guarded() chose was chosen FOR THE OLD WEIGHTS: back to the default plan until it is called again
            self.fp8_off, self.fp8_start, self.fp8_guard = False, None, None
        v = {k: np.asarray(a, np.float32) for k, a in variables.items() if k.startswith(p + '/')}
        check_variables(v, variable_shapes(p, self.cin, self.U, self.C))
        self.dense_deconv, deconv_scale, self.affine = {}, {}, {}
        for name, stride in (('upscore_conv5', 2), ('upscore', 8)):
            kern = dense_deconv_weights(v['%s/%s/kernel' % (p, name)], stride, self.U, self.Up, dev)
            if kern is not None:
                self.dense_deconv[name] = kern
            scale, affine = deconv_batch_norm(v, '%s/%s' % (p, name), self.U, self.Up, dev, kern is not None)
            if scale is not None:
                deconv_scale[name] = scale
            if affine is not None:
                self.affine[name] = affine
        self.w, self.b = {}, {}

        def folded(name):
            k, b = _fold_bn(v, '%s/%s' % (p, name), v['%s/%s/kernel' % (p, name)], v['%s/%s/bias' % (p, name)])
            if name == 'score_conv5' and 'upscore_conv5' in deconv_scale:
                # s*relu(up2(relu(z))) == relu(up2(relu(s*z))) for s > 0
                k, b = k * deconv_scale['upscore_conv5'], b * deconv_scale['upscore_conv5']
            return padded_score_conv(k, b, self.U, self.Up) if name.startswith('score_conv') else (k, b)

        for name in [e[0] for e in ENCODER] + ['score_conv4', 'score_conv5']:
            k, b = folded(name)
            self.w[name] = upload(k, dev) if name == 'conv1_1' else ops.pack_conv_weights(upload(k, dev))
            self.b[name] = upload(b, dev)
        k, b = _fold_bn(v, p + '/score', v[p + '/score/kernel'], v[p + '/score/bias'])
        k = k.reshape(self.U, self.C)
        if 'upscore' in deconv_scale:
            k = k * deconv_scale['upscore'][:, None]       # score(s*up) == (s-scaled score weights)(up)
        self.w['score'] = padded_score_matrix(k, self.Up, dev)
        self.b['score'] = upload(b, dev)
        if self.conv_dtype == 'fp8':
            # e4m3 images of the same (batch-norm folded) kernels, each with its own power-of-two scale
            self.w8, self.w8_exp = {}, {}
            for name in ('conv1_2', 'conv2_1') + FP8_CONVS + ('score_conv4', 'score_conv5'):
                self.w8[name], self.w8_exp[name] = ops.pack_conv_weights_f8(upload(folded(name)[0], dev))
        torch.cuda.synchronize(dev)

    # ---- fp8: static per-tensor scales -----------------------------------------------------------------------
    def calibrate(self, x, margin_bits=1, _implicit=False, method=None):
        """Choose the power-of-two scale of every fp8 activation map from one representative batch: run the bf16
        graph, take max|activation| per layer, and leave `margin_bits` of headroom (an e4m3 value keeps its 3
        mantissa bits anywhere in 2^-6 .. 2^8 of the scale, so headroom costs no precision; values beyond it
        saturate at 448 * 2^e).  Returns the exponents; they stay fixed until the next call (static calibration:
        no data-dependent work on the inference path)."""
        dtype, self.conv_dtype = self.conv_dtype, 'bf16'
        try:
            L = self.encoder(x, keep_all=True)
        finally:
            self.conv_dtype = dtype
        method = method or FP8_CALIBRATION
        if method == 'mse':
            # the exponent that minimises the map's squared e4m3 error (outliers saturate), not the one that fits its maximum
            self.fp8_scales = {name: ops.fp8_scale_exp_mse(L[name].interior(), margin_bits) for name in FP8_MAPS}
        else:
            self.fp8_scales = {name: ops.fp8_scale_exp(L[name].interior().abs().max().item(), margin_bits)
                               for name in FP8_MAPS}
        self._fp8_explicit = not _implicit
        return dict(self.fp8_scales)

    def calibrate_guarded(self, x, agreement=FP8_GUARD_AGREEMENT, candidates=FP8_GUARD_CANDIDATES, margin_bits=1, method=None):
        """calibrate(), then choose this expert's e4m3 plan BY ITS EFFECT: the label map of the calibration batch through the
        bf16 graph is the yardstick, and the plan becomes the deepest candidate (first e4m3 conv as early as possible) whose
        labels agree with it on at least `agreement` of the pixels; an expert that fails the bound with every candidate keeps
        bf16 operands (fp8_off).  One global plan was a guess: tools/fp8_calib_study.py -- a weak expert (the depth expert of
        the accuracy test: thresholds on one raw uint16 channel, 0.4 % of its pixels with a clear top-2 margin) flips 1.1-1.3 %
        of its labels under ANY e4m3 plan and loses up to half a point of mIoU, the RGB expert 0.2 % and nothing.  Costs a few
        forward passes at calibration time, nothing afterwards.  Returns the exponents; self.fp8_guard holds the report
        {'chosen', 'agreement': {candidate: fraction}, 'bound'}."""
        if self.conv_dtype != 'fp8':
            raise ValueError("calibrate_guarded: conv_dtype is %r" % self.conv_dtype)
        self.fp8_off = False
        scales = self.calibrate(x, margin_bits, method=method)
        self.fp8_off = True                                        # the yardstick: this engine on bf16 operands
        ref = self.forward(x, want=('label',))['label'].clone()
        self.fp8_off = False
        report, chosen = {}, 'bf16'
        for start in candidates:
            self.fp8_start = start
            lab = self.forward(x, want=('label',))['label']
            report[start] = float((lab == ref).float().mean().item())
            if report[start] >= agreement:
                chosen = start
                break
        if chosen == 'bf16':
            self.fp8_off, self.fp8_start = True, None
        self.fp8_guard = {'chosen': chosen, 'agreement': {k: round(v, 6) for k, v in report.items()}, 'bound': float(agreement)}
        return scales

    def _fp8_plan(self, x):
        if self.conv_dtype != 'fp8' or self.fp8_off:
            return (), ()
        if self.fp8_scales is None:
            self.calibrate(x, _implicit=True)           # first batch seen = calibration batch
        return fp8_plan(x.shape[1], x.shape[2], self.fp8_deep, self.fp8_start)

    def encoder(self, x, keep_all=False, routed=False):
        """x: float32 [N,H,W,cin] device tensor (raw 0..255 RGB / raw depth, data contract of
        xview/datasets/*) -> dict of Acts; 'fused' is the encoding (simple_fcn.py:10-87).
        keep_all=True also materialises every convX_Y / poolX like the reference's layer dict.
        routed=True (with keep_all; the training step): a conv in front of a pool whose full map only MaxPoolGrad would read
        leaves 'route_<name>' (uint8 route bytes, ops.conv2d_fwd_route) in the dict instead of '<name>', where the kernel
        takes the shape."""
        return self.encoder_finish(self.encoder_begin(x, keep_all=keep_all, stop=len(ENCODER), routed=routed))

    # The encoder in three steps (Vgg16Walk.encoder_begin, the remaining layers here or paired: encoder_layers_pair, and
    # encoder_finish: score convs, x2 upsampling + skip).
    def _drop_fn(self):
        return self._dropout if self.dropout_layers and self.dropout_rate > 0 else None

    def pairable(self):
        """May this engine's 3x3 layers share launches with a twin's (encoder_layers_pair)?"""
        return self.conv_dtype == 'bf16' and self._drop_fn() is None and self._sk() is None

    def encoder_finish(self, st):
        n, h, w = st['n'], st['h'], st['w']
        L = st['L']
        if 's4' in st:
            s4, s5 = st['s4'], st['s5']
        else:
            self.encoder_layers(st, len(ENCODER))
            drop = self._drop_fn()                        # (sites exist in the bf16 graph only: set_dropout)
            wts = self.w8 if st['convs8'] else self.w     # an fp8 plan ends in e4m3 conv4_3 / conv5_3 maps (fp8_plan)
            s4 = self._act('score_conv4', n, h // 8, w // 8, self.Up)
            c43 = drop(L['conv4_3'], 'conv4_3_drop') if drop is not None and 'conv4_3' in self.dropout_layers else L['conv4_3']
            ops.conv2d_fwd(c43, wts['score_conv4'], self.b['score_conv4'], 1, relu=True, y=s4)
            s5 = self._act('score_conv5', n, h // 16, w // 16, self.Up)
            c53 = drop(L['conv5_3'], 'conv5_3_drop') if drop is not None and 'conv5_3' in self.dropout_layers else L['conv5_3']
            ops.conv2d_fwd(c53, wts['score_conv5'], self.b['score_conv5'], 1, relu=True, y=s5)
        fused = upsample2x_skip(self, s5, s4, self._act('fused', n, h // 8, w // 8, self.Up),
                                self.dense_deconv.get('upscore_conv5'), self.affine.get('upscore_conv5'))
        L.update(score_conv4=s4, score_conv5=s5, fused=fused)
        if self.dropout_rate > 0 and 'features' in self.dropout_layers:
            # decoder(..., dropout_rate) drops its input features INSIDE the decoder (simple_fcn.py:124-126): the layer
            # dict keeps 'fused' undropped like the reference's, the head reads 'features_drop'
            L['features_drop'] = self._dropout(fused, 'features_drop')
        self._dropout_pass += 1
        return L

    def set_dropout(self, dropout_layers, dropout_rate, seed=0):
        """Enable (or, with an empty list / rate 0, disable) the MC-dropout sites of encoder / decoder."""
        if self.conv_dtype != 'bf16' and dropout_layers and dropout_rate > 0:
            raise NotImplementedError("dropout sites exist in the bf16 graph only (conv_dtype='fp8' is plain inference)")
        self.dropout_layers, self.dropout_rate, self.dropout_seed = tuple(dropout_layers), float(dropout_rate), int(seed)

    @staticmethod
    def _dropout_seed_of(dropout_seed, dropout_pass, tag):
        site = sum(ord(ch) for ch in tag)
        return (dropout_seed * 0x9E3779B1 + dropout_pass * 1000003 + site) & 0xffffffffffffffff

    def _dropout(self, x, tag):
        seed = self._dropout_seed_of(self.dropout_seed, self._dropout_pass, tag)
        return ops.dropout(x, self.dropout_rate, seed, y=self._act(tag, x.n, x.h, x.w, x.c))

    def mc_lowres_scores(self, x, num_samples, rate, seed, st=None):
        """The passes of the MC-dropout (variance fusion) model: the plain pass and `num_samples` passes with the dropout sites
        'pool3' (after pool3 and pool4) at `rate`, as low-resolution class scores float32 [(T+1) N][h/8+2][w/8+2][CP],
        slot-major (slot 0 the plain pass, slot t sample t; lowres_scores of each).  Everything up to pool3 is the same for
        all of them and runs ONCE; pool3 is then replicated into T + 1 slots (slot t dropped, ops.dropout_samples), and conv4_1
        on runs as one batch of (T+1) N images, pool4 dropped in place.  Sample t uses dropout pass p0 + t-1 with
        the seeds of _dropout (p0: the engine's pass counter, which advances by T): the bits of T sequential
        set_dropout(['pool3'], rate, seed) + lowres_scores passes.  Samples run in chunks of at most mc_chunk_images images
        per launch (each chunk with its own copy of the plain slot; masks are per sample, so chunking changes no bit).
        st: an encoder state (encoder_begin without dropout) to continue instead of `x`."""
        T = self._mc_check('mc_lowres_scores', num_samples)
        names = [e[0] for e in ENCODER]
        i41, i43 = names.index('conv4_1'), names.index('conv4_3')
        if st is None:
            st = self.encoder_begin(x, stop=i41)
        elif st['keep_all'] or st['next'] > i41:
            raise ValueError('mc_lowres_scores(st=...): an encoder state begun without keep_all, before conv4_1')
        self.encoder_layers(st, i41)
        n, h, w = st['n'], st['h'], st['w']
        pool3 = st['cur']
        cp = (self.C + 3) // 4 * 4
        key = ('mc_S', T, n, h // 8, w // 8)
        S = self._arena.get(key)
        if S is None:
            S = self._arena[key] = torch.zeros(((T + 1) * n, h // 8 + 2, w // 8 + 2, cp), dtype=torch.float32,
                                               device=self.device)
        per = max(1, int(self.mc_chunk_images) // n - 1)        # samples per chunk (+ the plain slot)
        p0 = self._dropout_pass
        a = 0
        while a < T:
            k = min(per, T - a)
            m = (k + 1) * n
            rep = self._act('pool3_mc', m, pool3.h, pool3.w, pool3.c)
            ops.dropout_samples(pool3, k, rate, self._dropout_seed_of(seed, p0 + a, 'pool3_drop'), 1000003, y=rep)
            sc = self._state(m, h, w, cur=rep, next=i41)
            self.encoder_layers(sc, i43 + 1)
            ops.dropout_samples(sc['cur'], k, rate, self._dropout_seed_of(seed, p0 + a, 'pool4_drop'), 1000003, in_place=True)
            f = self.encoder_finish(sc)['fused']
            if a == 0:
                ops.score_lowres(f, self.w['score'], self.C, S[:m])
            else:      # the samples alone; the chunk's plain slot repeats slot 0
                ops.score_lowres(f.images(n, m), self.w['score'], self.C, S[(1 + a) * n:(1 + a + k) * n])
            a += k
        self._dropout_pass = p0 + T
        return S, (n, h // 8, w // 8)

    def mc_input_scores(self, x, num_samples, rate, seed):
        """The passes of the uncertainty-weighted Dirichlet fusion (uncertainty_dirichlet_mix.py:106-127): the plain pass and
        `num_samples` passes on the INPUT with whole pixels dropped at `rate` (ops.dropout_pixels), as low-resolution class
        scores float32 [(T+1) N][h/8+2][w/8+2][CP], slot-major (slot 0 the plain pass, slot t sample t).  The site is the
        input, so nothing is shared between the passes: all T + 1 trunks run, the samples as batches of at most
        mc_chunk_images images.  Sample t carries the bits of pass p0 + t-1 run alone, lowres_scores(dropout_pixels(x, rate,
        _dropout_seed_of(seed, pass, 'input_drop'))) (p0: the engine's pass counter, which advances by T; masks are per sample,
        so chunking changes no bit)."""
        T = self._mc_check('mc_input_scores', num_samples)
        n, h, w, _ = x.shape
        x = x.contiguous()
        cp = (self.C + 3) // 4 * 4
        key = ('mci_S', T, n, h // 8, w // 8)
        S = self._arena.get(key)
        if S is None:
            S = self._arena[key] = torch.zeros(((T + 1) * n, h // 8 + 2, w // 8 + 2, cp), dtype=torch.float32,
                                               device=self.device)
        p0 = self._dropout_pass
        ops.score_lowres(self.encoder(x)['fused'], self.w['score'], self.C, S[:n])
        per = max(1, int(self.mc_chunk_images) // n)               # samples per chunk
        a = 0
        while a < T:
            k = min(per, T - a)
            ykey = ('mci_x', k * n, h, w)
            xs = self._arena.get(ykey)
            if xs is None:
                xs = self._arena[ykey] = torch.empty((k * n, h, w, self.cin), dtype=torch.float32, device=self.device)
            ops.dropout_pixels_samples(x, k, rate, self._dropout_seed_of(seed, p0 + a, 'input_drop'), 1000003, plain=False, y=xs)
            ops.score_lowres(self.encoder(xs)['fused'], self.w['score'], self.C, S[(1 + a) * n:(1 + a + k) * n])
            a += k
        self._dropout_pass = p0 + T
        return S, (n, h // 8, w // 8)

    def _mc_check(self, who, num_samples):
        """What the batched samplers refuse; returns T"""
        if self.conv_dtype != 'bf16':
            raise NotImplementedError("dropout sites exist in the bf16 graph only (conv_dtype='fp8' is plain inference)")
        if not self.commuted_head():
            raise NotImplementedError('%s needs the commuted decoder head (bilinear x8 deconv, no batch norm '
                                      'shift before its relu)' % who)
        if self._drop_fn() is not None:
            raise ValueError('%s draws its own masks: disable the dropout sites (set_dropout([], 0)) first' % who)
        T = int(num_samples)
        if T < 1:
            raise ValueError('num_samples must be at least 1')
        return T

    def mc_sample_scores(self, x, num_samples, rate, seed, dropout_layers, st=None):
        """The T = `num_samples` passes of the MC-dropout Bayesian FCN (bayesian_fcn.py:74-89): low-resolution class scores
        float32 [T N][h/8+2][w/8+2][CP], sample-major (images t N .. t N + N-1 are sample t; NO plain slot), each slot the BITS
        of pass p0 + t of set_dropout(dropout_layers, rate, seed) + lowres_scores(x) (p0: the engine's pass counter, which
        advances by T; seeds of _dropout, stride 1000003 per pass).  What all samples share runs once on N images, and the
        samples are replicated at the EARLIEST active site (ops.dropout_samples(sample_only=True): per-SAMPLE seeds inside one
        batch; later sites are dropped in place):
          'pool3' listed      conv1_1 .. pool3 once; pool3 replicated and dropped, conv4_1 on as one batch of T N images, pool4
                              dropped ('pool3' gates both pool dropouts, simple_fcn.py:51-63; 'pool4' alone enables nothing), then
                              conv4_3 (the full map in front of score_conv4; pool4 comes from the undropped one), conv5_3 and
                              the decoder's input features where listed;
          'pool3' not listed  the whole 3x3 trunk through conv5_3 once; conv4_3 -> score_conv4 and conv5_3 -> score_conv5 are
                              replicated where listed (dropped) or after their score conv (copies), then x2 upsample + add,
                              'features'; 'features' alone replicates the decoder's input only;
          no active site      (rate 0, or nothing but 'pool4'): T copies of the plain pass.
        Samples run in chunks of at most mc_chunk_images images per launch (masks are per sample: chunking changes no bit).
        st: an encoder state (encoder_begin without dropout and without keep_all) to continue instead of `x`."""
        T = self._mc_check('mc_sample_scores', num_samples)
        sites = set(dropout_layers) if float(rate) > 0 else set()
        pool, d43, d53, dfeat = ('pool3' in sites), ('conv4_3' in sites), ('conv5_3' in sites), ('features' in sites)
        names = [e[0] for e in ENCODER]
        i41, i43 = names.index('conv4_1'), names.index('conv4_3')
        shared = i41 if pool else len(ENCODER)
        if st is None:
            st = self.encoder_begin(x, stop=shared)
        elif st['keep_all'] or st['next'] > shared or 's4' in st:
            raise ValueError('mc_sample_scores(st=...): an encoder state begun without keep_all, before the first dropout site')
        self.encoder_layers(st, shared)
        n, h, w = st['n'], st['h'], st['w']
        hi, wi = h // 8, w // 8
        cp = (self.C + 3) // 4 * 4
        key = ('mcs_S', T, n, hi, wi)
        S = self._arena.get(key)
        if S is None:
            S = self._arena[key] = torch.zeros((T * n, hi + 2, wi + 2, cp), dtype=torch.float32, device=self.device)
        p0 = self._dropout_pass
        if not (pool or d43 or d53 or dfeat):
            S0, _ = self.lowres_scores(st=st)
            S.view((T, n) + tuple(S.shape[1:])).copy_(S0)
            self._dropout_pass = p0 + T
            return S, (n, hi, wi)

        def score_conv(src, name, m):
            y = self._act(name, m, src.h, src.w, self.Up)
            ops.conv2d_fwd(src, self.w[name], self.b[name], 1, relu=True, y=y)
            return y

        def finish(s4, s5, m):           # x2 upsample + skip of ready score maps (encoder_finish's own tail)
            return self.encoder_finish({'n': m, 'h': h, 'w': w, 'L': {}, 's4': s4, 's5': s5})['fused']

        once = {}
        if not pool:
            L = st['L']
            if not d43:
                once['s4'] = score_conv(L['conv4_3'], 'score_conv4', n)
            if not d53:
                once['s5'] = score_conv(L['conv5_3'], 'score_conv5', n)
            if not d43 and not d53:
                once['fused'] = finish(once['s4'], once['s5'], n)
        per = max(1, int(self.mc_chunk_images) // n)              # samples per chunk
        a = 0
        while a < T:
            k = min(per, T - a)
            m = k * n

            def drop(act, tag, src=None):
                """the chunk's k slots of `act` dropped in place, or (src: an n-image map) written from src"""
                ops.dropout_samples(act if src is None else src, k, rate, self._dropout_seed_of(seed, p0 + a, tag + '_drop'),
                                    1000003, y=None if src is None else act, in_place=src is None, sample_only=True)
                return act

            def slots(src, tag, dropped):
                y = self._act(tag + '_mc', m, src.h, src.w, src.c)
                if dropped:
                    return drop(y, tag, src=src)
                y.t.view((k, n) + tuple(y.t.shape[1:])).copy_(src.t)
                return y

            if pool:
                sc = self._state(m, h, w, cur=slots(st['cur'], 'pool3', True), next=i41)
                self.encoder_layers(sc, i43 + 1)
                drop(sc['cur'], 'pool4')
                self.encoder_layers(sc, len(ENCODER))
                if d43:
                    drop(sc['L']['conv4_3'], 'conv4_3')
                if d53:
                    drop(sc['L']['conv5_3'], 'conv5_3')
                f = self.encoder_finish(sc)['fused']
                if dfeat:
                    drop(f, 'features')
            elif 'fused' in once:
                f = slots(once['fused'], 'features', True)
            else:
                s4 = (score_conv(slots(L['conv4_3'], 'conv4_3', True), 'score_conv4', m) if d43
                      else slots(once['s4'], 'score_conv4', False))
                s5 = (score_conv(slots(L['conv5_3'], 'conv5_3', True), 'score_conv5', m) if d53
                      else slots(once['s5'], 'score_conv5', False))
                f = finish(s4, s5, m)
                if dfeat:
                    drop(f, 'features')
            ops.score_lowres(f, self.w['score'], self.C, S[a * n:(a + k) * n])
            a += k
        self._dropout_pass = p0 + T
        return S, (n, hi, wi)

    def commuted_head(self):
        """True if the decoder head runs in its commuted form (class scores interpolated at 1/8 resolution): no batch-norm
        shift between the x8 deconv and its relu, bilinear deconv kernel -- the precondition of `lowres_scores`."""
        return 'upscore' not in self.affine and 'upscore' not in self.dense_deconv

    def lowres_scores(self, x=None, st=None):
        """Trunk + the 1x1 score conv at 1/8 resolution: float32 [N][h/8+2][w/8+2][CP] (the first half of the decoder
        head, xv_score_lowres); the fused two-expert head of the fusion models takes it from here.  st: an encoder state
        (encoder_begin / encoder_layers_pair) to finish instead of an input."""
        L = self.encoder_finish(st) if st is not None else self.encoder(x)
        f = L.get('features_drop', L['fused'])
        cp = (self.C + 3) // 4 * 4
        key = ('lowres_S', f.n, f.h, f.w)
        S = self._arena.get(key)
        if S is None:
            S = self._arena[key] = torch.zeros((f.n, f.h + 2, f.w + 2, cp), dtype=torch.float32, device=self.device)
        ops.score_lowres(f, self.w['score'], self.C, S)
        return S, (f.n, f.h, f.w)

    def forward(self, x, want=('label',), keep_all=False, st=None):
        """fcn + test_pipeline (basic_fusion_model.py:9-23): returns dict with any of
        'score', 'prob' (float32 [N,H,W,C]) and 'label' == 'classification' (int64 [N,H,W])."""
        if st is not None and bool(keep_all) != bool(st['keep_all']):
            raise ValueError('forward(st=...): the encoder state was begun with keep_all=%r' % st['keep_all'])
        L = self.encoder_finish(st) if st is not None else self.encoder(x, keep_all=keep_all)
        f = L.get('features_drop', L['fused'])           # the decoder's input (dropped only when 'features' is a dropout site)
        key = ('head_ws', f.n, f.h, f.w)
        ws = self._arena.get(key)
        if ws is None:             # per-engine workspace: the two experts run on different streams
            ws = torch.empty(ops._lib.lib().xv_decoder_head_workspace_bytes(f.n, f.h, f.w, self.C) // 4,
                             dtype=torch.float32, device=self.device)
            self._arena[key] = ws
        out = decoder_head(self, f, want, self.dense_deconv.get('upscore'), self.affine.get('upscore'), L, workspace=ws)
        if 'label' in out:
            out['classification'] = out['label']
        out['layers'] = L
        return out
