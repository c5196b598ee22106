// On-device training augmentation for gfx950: the host chain of datasets/augmentation.py (scale, rotate + centre crop, shear,
// crop, flips, photometric table, label flip / merge, multiple-of-16 cut, float cast) for a whole batch in one launch, bit for
// bit.  Nothing intermediate exists in memory: an output pixel is pulled back through the stages, every stage value computed
// where it is needed (up to 4 x 4 x 4 source taps per output pixel; neighbours share them through the caches).
//
// Arithmetic: float64, in numpy's operation order (imageops.resize_linear / resize_nearest / warp_affine / _restore_dtype),
// contraction OFF for this whole file (the Makefile passes -ffp-contract=off; the pragma below says the same): every product
// and sum is then the IEEE double numpy forms, so the results EQUAL the host's.  rint is round-half-to-even, as np.rint.
#include "xv_common.h"

#pragma clang fp contract(off)

namespace {

// one pixel of every modality; integer values held as doubles between the stages (each stage rounds to its integer type, as
// the host chain stores uint8 / uint16 / int32 arrays between its steps)
struct Px {
  double r, g, b, d, l;
};

struct Pool {
  const uint8_t* rgb;      // the selected source image
  const uint16_t* depth;
  const int32_t* labels;
  int H, W;
};

__device__ __forceinline__ Px px_zero() { return Px{0.0, 0.0, 0.0, 0.0, 0.0}; }

// a * (1 - f) + b * f, numpy's order
__device__ __forceinline__ Px px_mix(const Px& a, const Px& b, double f) {
  const double g = 1.0 - f;
  return Px{a.r * g + b.r * f, a.g * g + b.g * f, a.b * g + b.b * f, a.d * g + b.d * f, a.l * g + b.l * f};
}

__device__ __forceinline__ double restore(double v, double lo, double hi) { return fmin(fmax(rint(v), lo), hi); }

// imageops._restore_dtype for uint8 rgb, uint16 depth, int32 labels
__device__ __forceinline__ Px px_restore(const Px& v) {
  return Px{restore(v.r, 0.0, 255.0), restore(v.g, 0.0, 255.0), restore(v.b, 0.0, 255.0), restore(v.d, 0.0, 65535.0),
            restore(v.l, -2147483648.0, 2147483647.0)};
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// floor()ed coordinate -> int; anything below -2 or above 2^30 is outside every image either way
__device__ __forceinline__ int coord_int(double fl) { return (int)fmin(fmax(fl, -2.0), 1073741824.0); }

// ---- stage 1: the scaled image (imageops.scale_image: rgb bilinear with half-pixel centres, depth and labels nearest) -------
__device__ __forceinline__ Px sample_scaled(const Pool& s, const xv_augment_plan& p, int y, int x) {
  Px out;
  if (!(p.stages & XVA_SCALE)) {
    const size_t at = (size_t)clampi(y, 0, s.H - 1) * s.W + clampi(x, 0, s.W - 1);
    out.r = s.rgb[at * 3], out.g = s.rgb[at * 3 + 1], out.b = s.rgb[at * 3 + 2];
    out.d = s.depth[at], out.l = s.labels[at];
    return out;
  }
  const double sy = ((double)y + 0.5) * p.scale_ry - 0.5, sx = ((double)x + 0.5) * p.scale_rx - 0.5;
  const double ly = floor(sy), lx = floor(sx);
  const double fr = sy - ly, fc = sx - lx;
  const int iy = coord_int(ly), ix = coord_int(lx);
  const size_t r0 = (size_t)clampi(iy, 0, s.H - 1) * s.W, r1 = (size_t)clampi(iy + 1, 0, s.H - 1) * s.W;
  const size_t c0 = clampi(ix, 0, s.W - 1), c1 = clampi(ix + 1, 0, s.W - 1);
  const uint8_t *p00 = s.rgb + (r0 + c0) * 3, *p01 = s.rgb + (r0 + c1) * 3, *p10 = s.rgb + (r1 + c0) * 3,
                *p11 = s.rgb + (r1 + c1) * 3;
  const double gc = 1.0 - fc, gr = 1.0 - fr;
  out.r = restore(((double)p00[0] * gc + (double)p01[0] * fc) * gr + ((double)p10[0] * gc + (double)p11[0] * fc) * fr, 0.0, 255.0);
  out.g = restore(((double)p00[1] * gc + (double)p01[1] * fc) * gr + ((double)p10[1] * gc + (double)p11[1] * fc) * fr, 0.0, 255.0);
  out.b = restore(((double)p00[2] * gc + (double)p01[2] * fc) * gr + ((double)p10[2] * gc + (double)p11[2] * fc) * fr, 0.0, 255.0);
  // resize_nearest: index = int(dst * (n_in / n_out)), capped at the last one
  const int ny = clampi((int)((double)y * p.scale_ry), 0, s.H - 1), nx = clampi((int)((double)x * p.scale_rx), 0, s.W - 1);
  const size_t at = (size_t)ny * s.W + nx;
  out.d = s.depth[at], out.l = s.labels[at];
  return out;
}

// imageops.warp_affine at destination pixel (X, Y): the four taps around (sx, sy) of an h x w image given by `fetch`, zero
// outside, blended as (f00 (1-fx) + f01 fx) (1-fy) + (f10 (1-fx) + f11 fx) fy and rounded to the integer types.  The tap loop
// stays rolled: one copy of the stage below per level, and the selects keep its four values out of indexed arrays.
template <class F>
__device__ __forceinline__ Px warp_taps(double a, double b, double c, double d, double e, double f, int X, int Y, int h, int w,
                                        F fetch) {
  const double sx = a * (double)X + b * (double)Y + c;
  const double sy = d * (double)X + e * (double)Y + f;
  const double lx = floor(sx), ly = floor(sy);
  const double fx = sx - lx, fy = sy - ly;
  const int x0 = coord_int(lx), y0 = coord_int(ly);
  Px left = px_zero(), top = px_zero(), out = px_zero();
#pragma unroll 1
  for (int t = 0; t < 4; ++t) {
    const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
    Px v = px_zero();
    if (yy >= 0 && yy < h && xx >= 0 && xx < w) v = fetch(yy, xx);
    if (!(t & 1)) {
      left = v;
    } else {
      const Px row = px_mix(left, v, fx);
      if (t == 1)
        top = row;
      else
        out = px_mix(top, row, fy);
    }
  }
  return px_restore(out);
}

// ---- stage 2: the rotated image, cut to the centred inscribed rectangle (_rotated_canvas + _centre_crop) ----------------------
__device__ __forceinline__ Px sample_rotated(const Pool& s, const xv_augment_plan& p, int y, int x) {
  if (!(p.stages & XVA_ROTATE)) return sample_scaled(s, p, y, x);
  return warp_taps(p.rot_a, p.rot_b, p.rot_c, p.rot_d, p.rot_e, p.rot_f, x + p.rot_left, y + p.rot_top, p.scale_h, p.scale_w,
                   [&](int yy, int xx) { return sample_scaled(s, p, yy, xx); });
}

// ---- stage 3: the sheared image (_shear) ---------------------------------------------------------------------------------------
__device__ __forceinline__ Px sample_sheared(const Pool& s, const xv_augment_plan& p, int y, int x) {
  if (!(p.stages & XVA_SHEAR)) return sample_rotated(s, p, y, x);
  return warp_taps(p.shear_a, p.shear_b, p.shear_c, p.shear_d, p.shear_e, p.shear_f, x, y, p.rot_h, p.rot_w,
                   [&](int yy, int xx) { return sample_rotated(s, p, yy, xx); });
}

// One thread = one output pixel, x fastest inside a 16 x 16 tile (a wave = 4 rows of 16: compact source footprints);
// blockIdx.x = tile, blockIdx.y = output image, so the plan and every stage branch are wave-uniform.  S is a multiple of 16.
__global__ __launch_bounds__(256) void augment_batch_kernel(const uint8_t* __restrict__ rgb, const uint16_t* __restrict__ depth,
                                                           const int32_t* __restrict__ labels, int H, int W,
                                                           const int32_t* __restrict__ index,
                                                           const xv_augment_plan* __restrict__ plans,
                                                           const uint8_t* __restrict__ luts, int S, float* __restrict__ out_rgb,
                                                           float* __restrict__ out_depth, int32_t* __restrict__ out_labels) {
  const int img = blockIdx.y, tiles = S >> 4;
  const int ox = (blockIdx.x % tiles) * 16 + (threadIdx.x & 15), oy = (blockIdx.x / tiles) * 16 + (threadIdx.x >> 4);
  const xv_augment_plan& p = plans[img];
  const size_t src = (size_t)index[img] * H * W;
  const Pool s{rgb + src * 3, depth + src, labels + src, H, W};
  // back through the flips (np.flip of the crop_size^2 window; crop_multiple then keeps its first S rows / columns) and the crop
  const int y = p.crop_top + ((p.stages & XVA_FLIP_ROWS) ? p.crop_size - 1 - oy : oy);
  const int x = p.crop_left + ((p.stages & XVA_FLIP_COLS) ? p.crop_size - 1 - ox : ox);
  const Px v = sample_sheared(s, p, y, x);
  const uint8_t* lut = luts + (size_t)img * 256;
  int lab = (int)v.l;
  if ((p.stages & XVA_LABEL_FLIP) && lab == p.flip_from) lab = p.flip_to;
  if ((p.stages & XVA_LABEL_MERGE) && lab == p.merge_drop) lab = p.merge_keep;
  const size_t o = ((size_t)img * S + oy) * S + ox;
  out_rgb[o * 3] = (float)lut[(int)v.r], out_rgb[o * 3 + 1] = (float)lut[(int)v.g], out_rgb[o * 3 + 2] = (float)lut[(int)v.b];
  out_depth[o] = (float)v.d;
  out_labels[o] = lab;
}

// Is this plan one the kernel may run at source size H x W and output size S?  Every window has to lie inside the image of
// its stage (the kernel clamps source reads regardless; a plan that fails here would give values the host chain never gives).
bool plan_ok(const xv_augment_plan& p, int H, int W, int S) {
  int h = H, w = W;
  if (p.stages & ~(XVA_SCALE | XVA_ROTATE | XVA_SHEAR | XVA_FLIP_ROWS | XVA_FLIP_COLS | XVA_LABEL_FLIP | XVA_LABEL_MERGE))
    return false;
  if (p.stages & XVA_SCALE) {
    if (p.scale_h <= 0 || p.scale_w <= 0 || p.scale_h >= (1 << 24) || p.scale_w >= (1 << 24)) return false;
    if (!(p.scale_ry > 0.0) || !(p.scale_rx > 0.0) || !isfinite(p.scale_ry) || !isfinite(p.scale_rx)) return false;
  } else if (p.scale_h != h || p.scale_w != w) {
    return false;
  }
  h = p.scale_h, w = p.scale_w;
  if (p.stages & XVA_ROTATE) {
    if (p.canvas_h <= 0 || p.canvas_w <= 0 || p.canvas_h >= (1 << 24) || p.canvas_w >= (1 << 24)) return false;
    if (p.rot_top < 0 || p.rot_left < 0 || p.rot_h <= 0 || p.rot_w <= 0) return false;
    if ((int64_t)p.rot_top + p.rot_h > p.canvas_h || (int64_t)p.rot_left + p.rot_w > p.canvas_w) return false;
    for (double m : {p.rot_a, p.rot_b, p.rot_c, p.rot_d, p.rot_e, p.rot_f})
      if (!isfinite(m)) return false;
  } else if (p.rot_h != h || p.rot_w != w) {
    return false;
  }
  h = p.rot_h, w = p.rot_w;
  if (p.stages & XVA_SHEAR)
    for (double m : {p.shear_a, p.shear_b, p.shear_c, p.shear_d, p.shear_e, p.shear_f})
      if (!isfinite(m)) return false;
  if (p.crop_size < S || p.crop_top < 0 || p.crop_left < 0) return false;
  return (int64_t)p.crop_top + p.crop_size <= h && (int64_t)p.crop_left + p.crop_size <= w;
}

}  // namespace

extern "C" size_t xv_augment_plan_bytes(void) { return sizeof(xv_augment_plan); }

extern "C" int xv_augment_batch(const uint8_t* rgb, const uint16_t* depth, const int32_t* labels, int M, int H, int W,
                                const int32_t* index, const int32_t* index_host, const xv_augment_plan* plans,
                                const xv_augment_plan* plans_host, const uint8_t* luts, int N, int S, float* out_rgb,
                                float* out_depth, int32_t* out_labels, void* stream) {
  XV_CHECK_ARG(rgb && depth && labels && index && index_host && plans && plans_host && luts && out_rgb && out_depth &&
               out_labels);
  XV_CHECK_ARG(M > 0 && H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24));
  XV_CHECK_ARG(N > 0 && N <= 65535 && S > 0 && S % 16 == 0 && S <= (1 << 15));
  for (int n = 0; n < N; ++n) {
    XV_CHECK_ARG(index_host[n] >= 0 && index_host[n] < M);
    XV_CHECK_ARG(plan_ok(plans_host[n], H, W, S));
  }
  const dim3 grid((unsigned)((S >> 4) * (S >> 4)), (unsigned)N);
  hipLaunchKernelGGL(augment_batch_kernel, grid, dim3(256), 0, (hipStream_t)stream, rgb, depth, labels, H, W, index, plans, luts,
                     S, out_rgb, out_depth, out_labels);
  return xv_launch_status();
}
