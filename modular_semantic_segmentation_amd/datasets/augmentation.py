"""Training-time augmentation of an image blob and the multiple-of-16 crop of the data contract.

Host-side counterpart of the reference's `xview/datasets/augmentation.py` (`augmentate` :143-241,
`crop_multiple` :244-262) on numpy only: cv2 resampling is restated in `imageops`, the two imgaug
operators the reference uses are the plain formulas below.  The order of the transforms, their
argument convention (`[probability, low, high]` lists, `False` = off) and which random generator
each draw comes from (`random` vs `numpy.random`) follow the reference, so a seeded run takes the
same decisions.
"""
import math
import random

import numpy as np

from . import imageops


def crop_multiple(data, multiple_of=16):
    """Cut the two leading axes down to multiples of `multiple_of` (augmentation.py:244-262); things
    without a shape pass through."""
    shape = getattr(data, 'shape', None)
    if shape is None or len(shape) < 2:
        return data
    h, w = (int(d) - int(d) % multiple_of for d in shape[:2])
    if (h, w) == tuple(shape[:2]):
        return data
    return data[:h, :w, ...]


def _rotation_matrix(h, w, degrees):
    """(forward 2x3 matrix, canvas width, canvas height) of a rotation about the centre onto a canvas that holds the whole
    rotated h x w image (augmentation.py:8-76)."""
    rad = math.radians(degrees)
    a, b = math.cos(rad), math.sin(rad)
    cx, cy = w / 2.0, h / 2.0
    rot = np.array([[a, b, (1 - a) * cx - b * cy],
                    [-b, a, b * cx + (1 - a) * cy]])
    new_w = int(abs(w * a) + abs(h * b))
    new_h = int(abs(w * b) + abs(h * a))
    rot[0, 2] += int(new_w * 0.5 - w * 0.5)
    rot[1, 2] += int(new_h * 0.5 - h * 0.5)
    return rot, new_w, new_h


def _rotated_canvas(image, degrees):
    """Rotate about the centre onto the canvas of `_rotation_matrix`.  Every modality, labels included, is resampled
    bilinearly there; kept."""
    rot, new_w, new_h = _rotation_matrix(*image.shape[:2], degrees)
    return imageops.warp_affine(image, rot, new_w, new_h)


def inscribed_rect(w, h, radians):
    """Width and height of the axis-aligned rectangle the reference cuts out of a rotated w x h image
    (`largest_rotated_rect`, augmentation.py:79-116).  The reference's third angle is atan2(bb_w, bb_w),
    i.e. always 45 degrees, whatever the aspect ratio; reproduced because it decides the crop size."""
    quadrant = int(math.floor(radians / (math.pi / 2))) & 3
    alpha = radians if quadrant % 2 == 0 else math.pi - radians
    alpha = (alpha % math.pi + math.pi) % math.pi
    box_w = w * math.cos(alpha) + h * math.sin(alpha)
    box_h = w * math.sin(alpha) + h * math.cos(alpha)
    gamma = math.pi / 4
    delta = math.pi - alpha - gamma
    longest = max(w, h)
    a = longest * math.cos(alpha) * math.sin(alpha) / math.sin(delta)
    y = a * math.cos(gamma)
    x = y * math.tan(gamma)
    return box_w - 2 * x, box_h - 2 * y


def _centre_crop_bounds(h, w, width, height):
    """(row start, row stop, column start, column stop) of the centred window of at most width x height in an h x w image."""
    width, height = min(width, w), min(height, h)
    cx, cy = int(w * 0.5), int(h * 0.5)
    return int(cy - height * 0.5), int(cy + height * 0.5), int(cx - width * 0.5), int(cx + width * 0.5)


def _centre_crop(image, width, height):
    y0, y1, x0, x1 = _centre_crop_bounds(*image.shape[:2], width, height)
    return image[y0:y1, x0:x1]


def _shear_matrix(h, w, degrees):
    t = math.tan(math.radians(degrees))
    return np.array([[1.0, -t, t * h / 2.0], [0.0, 1.0, 0.0]])


def _shear(image, degrees):
    """Horizontal shear about the image centre, zero border (imgaug `Affine(shear=...)`)."""
    h, w = image.shape[:2]
    return imageops.warp_affine(image, _shear_matrix(h, w, degrees), w, h)


def _as_uint8(values):
    return np.clip(np.rint(values), 0, 255).astype(np.uint8)


def _flip_labels(labels, c1, c2, to_c2):
    if to_c2:
        labels[labels == c1] = c2
    else:
        labels[labels == c2] = c1
    return labels


def flip_labels(labels, c1, c2, prob=0.5):
    """Map c1 onto c2 with probability `prob`, else c2 onto c1 (augmentation.py:132-140)."""
    return _flip_labels(labels, c1, c2, np.random.rand() < prob)


def draw_augmentation(height, width, has_rgb=True, scale=False, crop=False, hflip=False, vflip=False, gamma=False,
                      contrast=False, brightness=False, rotate=False, shear=False, label_flip=False, label_merge=False):
    """Every random decision `augmentate` takes for a height x width sample, as a plan of plain host numbers.

    `random` and `numpy.random` are consumed exactly as `augmentate` consumes them: same generator per draw, same order, same
    short circuits (`has_rgb`: the photometric draws are only taken for a blob with an 'rgb' modality).  The image size is
    tracked through the stages because later draws depend on it.  A stage that is not drawn is None (a flag: False).

    scale        {'k', 'size': (h, w) after it, 'ratio': (h_in / h_out, w_in / w_out) as `imageops.resize_*` form them}
    rotate       {'degrees', 'canvas': (h, w), 'inverse': 2x3 float64 list, destination -> source as `warp_affine` inverts it,
                  'crop': (top, left, h, w) of the centred inscribed rectangle on the canvas}
    shear        {'degrees', 'inverse': 2x3}
    crop         {'top', 'left', 'size'}
    hflip, vflip reverse axis 0 / axis 1 (the reference's naming)
    contrast     alpha; brightness: offset; gamma: k
    label_flip   (from, to); label_merge: (keep, drop)
    size         (h, w) of the result
    """
    h, w = int(height), int(width)
    plan = {'input_size': (h, w), 'scale': None, 'rotate': None, 'shear': None, 'crop': None, 'hflip': False,
            'vflip': False, 'contrast': None, 'brightness': None, 'gamma': None, 'label_flip': None, 'label_merge': None}
    do_crop = bool(crop) and crop[0] > random.random()

    if scale and do_crop and scale[0] > random.random():
        k = random.uniform(max(crop[1] / float(min(h, w)), scale[1]), scale[2])
        out_h, out_w = int(round(h * k)), int(round(w * k))                  # imageops.scale_image
        plan['scale'] = {'k': k, 'size': (out_h, out_w), 'ratio': (h / out_h, w / out_w)}
        h, w = out_h, out_w

    if rotate and rotate[0] > random.random():
        degrees = np.random.randint(rotate[1], rotate[2])
        rot, canvas_w, canvas_h = _rotation_matrix(h, w, degrees)
        y0, y1, x0, x1 = _centre_crop_bounds(canvas_h, canvas_w, *inscribed_rect(w, h, math.radians(degrees)))
        y1, x1 = min(y1, canvas_h), min(x1, canvas_w)                        # what the slice keeps
        plan['rotate'] = {'degrees': degrees, 'canvas': (canvas_h, canvas_w),
                          'inverse': imageops.invert_affine(rot)[:2].tolist(),
                          'crop': (y0, x0, max(y1 - y0, 0), max(x1 - x0, 0))}
        h, w = plan['rotate']['crop'][2:]

    if shear and do_crop and shear[0] > random.random():
        amount = np.random.randint(shear[1] * w, shear[2] * w) * np.random.choice([-1, 1])
        plan['shear'] = {'degrees': amount, 'inverse': imageops.invert_affine(_shear_matrix(h, w, amount))[:2].tolist()}

    if do_crop:
        top = random.randint(0, h - crop[1])
        left = random.randint(0, w - crop[1])
        plan['crop'] = {'top': top, 'left': left, 'size': crop[1]}
        h = w = crop[1]

    plan['hflip'] = bool(hflip and hflip > random.random() and np.random.choice([0, 1]))
    plan['vflip'] = bool(vflip and vflip > random.random() and np.random.choice([0, 1]))

    if contrast and has_rgb and contrast[0] > np.random.rand():
        plan['contrast'] = np.random.uniform(contrast[1], contrast[2])
    if brightness and has_rgb and brightness[0] > np.random.rand():
        plan['brightness'] = np.random.randint(brightness[1], brightness[2] + 1)
    if gamma and has_rgb and gamma[0] > random.random():
        plan['gamma'] = random.uniform(gamma[1], gamma[2])

    if label_flip:
        c1, c2 = label_flip
        plan['label_flip'] = (c1, c2) if np.random.rand() < 0.5 else (c2, c1)
    if label_merge:
        plan['label_merge'] = (label_merge[0], label_merge[1])
    plan['size'] = (h, w)
    return plan


def _contrast(values, alpha):
    return _as_uint8(128.0 + alpha * (values.astype(np.float64) - 128.0))


def _brightness(values, offset):
    return _as_uint8(values.astype(np.float64) + offset)


def _gamma(values, k):
    lut = (((np.arange(256) / 255.0) ** (1 / k)) * 255).astype('uint8')
    return lut[values]


def photometric_table(plan):
    """The plan's contrast, brightness and gamma, each a uint8 -> uint8 map, composed in that order into one 256-entry uint8
    table by the formulas `apply_augmentation` applies to the image: table[rgb] is what the three steps make of rgb."""
    table = np.arange(256, dtype=np.uint8)
    if plan['contrast'] is not None:
        table = _contrast(table, plan['contrast'])
    if plan['brightness'] is not None:
        table = _brightness(table, plan['brightness'])
    if plan['gamma'] is not None:
        table = _gamma(table, plan['gamma'])
    return table


def apply_augmentation(blob, plan):
    """Carry out a plan of `draw_augmentation` on all modalities of one sample; draws nothing."""
    modalities = list(blob.keys())

    if plan['scale'] is not None:
        for m in modalities:
            blob[m] = imageops.scale_image(blob[m], plan['scale']['k'], nearest=(m != 'rgb'))

    if plan['rotate'] is not None:
        h, w = blob[modalities[0]].shape[:2]
        degrees = plan['rotate']['degrees']
        rect = inscribed_rect(w, h, math.radians(degrees))
        for m in modalities:
            blob[m] = _centre_crop(_rotated_canvas(blob[m], degrees), *rect)

    if plan['shear'] is not None:
        for m in modalities:
            blob[m] = _shear(blob[m], plan['shear']['degrees'])

    if plan['crop'] is not None:
        top, left, size = (plan['crop'][k] for k in ('top', 'left', 'size'))
        for m in modalities:
            blob[m] = blob[m][top:top + size, left:left + size, ...]

    if plan['hflip']:
        for m in modalities:
            blob[m] = np.flip(blob[m], axis=0)

    if plan['vflip']:
        for m in modalities:
            blob[m] = np.flip(blob[m], axis=1)

    if plan['contrast'] is not None:
        blob['rgb'] = _contrast(blob['rgb'], plan['contrast'])

    if plan['brightness'] is not None:
        blob['rgb'] = _brightness(blob['rgb'], plan['brightness'])

    if plan['gamma'] is not None:
        blob['rgb'] = _gamma(blob['rgb'], plan['gamma'])

    if plan['label_flip'] is not None:
        c_from, c_to = plan['label_flip']
        blob['labels'][blob['labels'] == c_from] = c_to

    if plan['label_merge'] is not None:
        blob['labels'][blob['labels'] == plan['label_merge'][1]] = plan['label_merge'][0]

    return blob


def augmentate(blob, scale=False, crop=False, hflip=False, vflip=False, gamma=False, contrast=False,
               brightness=False, rotate=False, shear=False, label_flip=False, label_merge=False):
    """Augment all modalities of one sample consistently (augmentation.py:143-241): `draw_augmentation` for the sample's
    size, then `apply_augmentation`.

    scale [p, lo, hi]: resize by a factor from [max(lo, crop/min side), hi], only when cropping;
    crop [p, size]: random size x size window; rotate [p, lo_deg, hi_deg]; shear [p, lo, hi]
    (fractions of the width, only when cropping); hflip / vflip: probability (the reference's hflip
    reverses axis 0 and vflip axis 1, each halved by a second coin; kept); gamma [p, lo, hi],
    contrast [p, lo, hi], brightness [p, lo, hi]: rgb only; label_flip [c1, c2]; label_merge [keep, drop].
    """
    h, w = blob[next(iter(blob))].shape[:2]
    return apply_augmentation(blob, draw_augmentation(
        h, w, has_rgb='rgb' in blob, scale=scale, crop=crop, hflip=hflip, vflip=vflip, gamma=gamma, contrast=contrast,
        brightness=brightness, rotate=rotate, shear=shear, label_flip=label_flip, label_merge=label_merge))
