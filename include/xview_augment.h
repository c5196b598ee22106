/* The plan record of xv_augment_batch (include/xview_hip.h): one per output image, what
 * datasets/augmentation.py::draw_augmentation drew for it, as the kernel reads it.  This is the only definition of the
 * layout: csrc/augment.hip includes it, datasets/device_augmentation.py derives its numpy record from this text and
 * checks the size against xv_augment_plan_bytes().  Members are doubles and int32_t only, doubles first (no padding).
 *
 * Stage chain, source -> output: scale -> rotate (+ centre crop) -> shear -> crop -> flips -> first S rows / columns.
 * `stages` says which are present (XVA_* bits below); the members of an absent stage are ignored, except that its
 * output size is its input size.  Image sizes: source H x W (arguments of the call); scaled scale_h x scale_w (H x W
 * without XVA_SCALE); rotated rot_h x rot_w, the window at (rot_top, rot_left) of the canvas_h x canvas_w canvas
 * (scale_h x scale_w without XVA_ROTATE); the shear keeps that size; the crop is the crop_size^2 window at (crop_top,
 * crop_left) of it.  The matrices are destination -> source, row-major 2x3: sx = a x + b y + c, sy = d x + e y + f.  */
#ifndef XVIEW_AUGMENT_H
#define XVIEW_AUGMENT_H
#include <stdint.h>

#define XVA_SCALE 1        /* bits of `stages` */
#define XVA_ROTATE 2
#define XVA_SHEAR 4
#define XVA_FLIP_ROWS 8    /* 'hflip' of the configuration: axis 0 reversed */
#define XVA_FLIP_COLS 16   /* 'vflip': axis 1 reversed */
#define XVA_LABEL_FLIP 32
#define XVA_LABEL_MERGE 64

typedef struct xv_augment_plan {
  double scale_ry, scale_rx;                                /* H / scale_h, W / scale_w, divided on the host */
  double rot_a, rot_b, rot_c, rot_d, rot_e, rot_f;          /* canvas pixel -> scaled image */
  double shear_a, shear_b, shear_c, shear_d, shear_e, shear_f;
  int32_t stages;
  int32_t scale_h, scale_w;
  int32_t canvas_h, canvas_w;
  int32_t rot_top, rot_left, rot_h, rot_w;
  int32_t crop_top, crop_left, crop_size;
  int32_t flip_from, flip_to;                               /* labels == flip_from become flip_to */
  int32_t merge_keep, merge_drop;                           /* then labels == merge_drop become merge_keep */
} xv_augment_plan;

#endif /* XVIEW_AUGMENT_H */
