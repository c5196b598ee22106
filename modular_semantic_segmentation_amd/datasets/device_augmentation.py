"""Training batches augmented on the device: `augmentation.augmentate`'s chain for a whole batch in one kernel launch
(`ops.augment_batch`, csrc/augment.hip), bit for bit what the host chain computes.

The sources stay resident in HBM as raw uint8 / uint16 / int32 images.  Per batch the host only draws: `draw_augmentation`
once per item, in item order, so `random` and `numpy.random` are consumed exactly as the host stream consumes them and a
seeded `DeviceTrainset` yields the batches a seeded host stream yields.  The drawn plans are packed into the records of
include/xview_augment.h, which is the one definition of their layout: the numpy record type below is read from that header.
"""
import os
import re

import numpy as np

from .augmentation import draw_augmentation, photometric_table

PLAN_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'include',
                           'xview_augment.h')
_NUMPY_OF = {'double': 'f8', 'int32_t': 'i4'}


def _read_plan_header():
    from .._lib import parse_header
    with open(PLAN_HEADER) as f:
        text = f.read()
    members = parse_header(text)[2]['xv_augment_plan']
    bits = {name: int(value) for name, value in re.findall(r'^#define (XVA_\w+) (\d+)', text, re.M)}
    return np.dtype([(name, _NUMPY_OF[ctype]) for name, ctype in members], align=True), bits


# numpy record of one xv_augment_plan; the XVA_* bits of its `stages` member
PLAN_DTYPE, STAGE_BITS = _read_plan_header()


def pack_plans(plans, height, width):
    """`draw_augmentation` plans of height x width samples -> record array [len(plans)] of xv_augment_plan.  Every plan must
    crop (the kernel writes square outputs of one size)."""
    out = np.zeros(len(plans), dtype=PLAN_DTYPE)
    for rec, plan in zip(out, plans):
        if plan['crop'] is None or tuple(plan['input_size']) != (height, width):
            raise ValueError('a plan without a crop, or drawn for another source size than %d x %d' % (height, width))
        stages, h, w = 0, height, width
        if plan['scale'] is not None:
            stages |= STAGE_BITS['XVA_SCALE']
            h, w = plan['scale']['size']
            rec['scale_ry'], rec['scale_rx'] = plan['scale']['ratio']
        rec['scale_h'], rec['scale_w'] = h, w
        if plan['rotate'] is not None:
            stages |= STAGE_BITS['XVA_ROTATE']
            rec['canvas_h'], rec['canvas_w'] = plan['rotate']['canvas']
            rec['rot_top'], rec['rot_left'], h, w = plan['rotate']['crop']
            for name, value in zip('abcdef', np.ravel(plan['rotate']['inverse'])):
                rec['rot_' + name] = value
        rec['rot_h'], rec['rot_w'] = h, w
        if plan['shear'] is not None:
            stages |= STAGE_BITS['XVA_SHEAR']
            for name, value in zip('abcdef', np.ravel(plan['shear']['inverse'])):
                rec['shear_' + name] = value
        rec['crop_top'], rec['crop_left'], rec['crop_size'] = (plan['crop'][k] for k in ('top', 'left', 'size'))
        stages |= STAGE_BITS['XVA_FLIP_ROWS'] if plan['hflip'] else 0
        stages |= STAGE_BITS['XVA_FLIP_COLS'] if plan['vflip'] else 0
        if plan['label_flip'] is not None:
            stages |= STAGE_BITS['XVA_LABEL_FLIP']
            rec['flip_from'], rec['flip_to'] = plan['label_flip']
        if plan['label_merge'] is not None:
            stages |= STAGE_BITS['XVA_LABEL_MERGE']
            rec['merge_keep'], rec['merge_drop'] = plan['label_merge']
        rec['stages'] = stages
    return out


def pack_tables(plans):
    """uint8 [len(plans), 256]: every plan's composed contrast -> brightness -> gamma table."""
    return np.stack([photometric_table(plan) for plan in plans])


class DeviceTrainset:
    """An endless stream of augmented training batches made on the device.

    pool    {'rgb': uint8 [M,H,W,3], 'depth': uint16 [M,H,W] or [M,H,W,1], 'labels': int32 [M,H,W]}: numpy arrays or lists
            of per-image arrays (uploaded once), or torch tensors that are already resident
    config  the keyword arguments of `augmentation.augmentate`
    `BaseModel.fit` takes its batches from `training_batches` when it is handed one of these."""

    modalities = ('rgb', 'depth', 'labels')
    _dtypes = {'rgb': np.uint8, 'depth': np.uint16, 'labels': np.int32}

    def __init__(self, pool, config, device='cuda'):
        import torch
        self.config = dict(config)
        crop = self.config.get('crop', False)
        if not crop:
            raise ValueError('device augmentation needs the crop: without it the images of a batch differ in size')
        if crop[0] < 1:
            raise ValueError('device augmentation needs crop probability 1 (got %s): an uncropped image has another size '
                             'than the cropped ones of its batch' % (crop[0],))
        self.device = torch.device(device)
        self.pool = {}
        for m in self.modalities:
            v = pool[m]
            if isinstance(v, torch.Tensor):
                t = v
            else:
                if isinstance(v, (list, tuple)):
                    shapes = sorted({tuple(np.shape(a)) for a in v})
                    if len(shapes) != 1:
                        raise ValueError("the '%s' sources are not all one size: %s" % (m, shapes))
                    v = np.stack([np.asarray(a) for a in v])
                v = np.asarray(v)
                if v.dtype != self._dtypes[m]:
                    raise ValueError("'%s' sources must be raw %s, not %s" % (m, np.dtype(self._dtypes[m]).name, v.dtype))
                t = torch.from_numpy(np.ascontiguousarray(v))
            self.pool[m] = t.to(self.device).contiguous()
        sizes = {m: tuple(t.shape[:3]) for m, t in self.pool.items()}
        if len(set(sizes.values())) != 1:
            raise ValueError('the sources are not all one size: %s' % sizes)
        self.num_items, self.height, self.width = sizes['rgb']
        if self.num_items < 1:
            raise ValueError('an empty pool')

    def __len__(self):
        return self.num_items

    def draw_batch(self, items):
        """(plans, record array, tables) for these pool items: one `draw_augmentation` per item, in order."""
        plans = [draw_augmentation(self.height, self.width, **self.config) for _ in items]
        return plans, pack_plans(plans, self.height, self.width), pack_tables(plans)

    def training_batches(self, batchsize):
        """Endless iterator of {'rgb': float32 [B,S,S,3], 'depth': float32 [B,S,S,1], 'labels': int32 [B,S,S]} device tensors:
        the next `batchsize` items in order, wrapping at the end of the pool; one upload and one launch per batch."""
        from .. import ops
        start = 0
        while True:
            items = (start + np.arange(batchsize)) % self.num_items
            start = (start + batchsize) % self.num_items
            _, records, tables = self.draw_batch(items)
            rgb, depth, labels = ops.augment_batch(self.pool, items.astype(np.int32), records, tables)
            yield {'rgb': rgb, 'depth': depth, 'labels': labels}
