// HBM-bound pointwise layers of the FCN for gfx950: max-pool, bilinear x2 (+add), depth-to-space, dropout, concat.
#include <stdlib.h>

#include "xv_common.h"

#pragma clang fp contract(on)  // by the source expression only, as in heads.hip

namespace {

__device__ inline u32x4 bf16x8_max(u32x4 a, u32x4 b) {
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float alo = bf16_bits_to_f32(a[i] & 0xffffu), ahi = __builtin_bit_cast(float, a[i] & 0xffff0000u);
    const float blo = bf16_bits_to_f32(b[i] & 0xffffu), bhi = __builtin_bit_cast(float, b[i] & 0xffff0000u);
    const uint32_t lo = __builtin_bit_cast(uint32_t, fmaxf(alo, blo)) >> 16;
    const uint32_t hi = __builtin_bit_cast(uint32_t, fmaxf(ahi, bhi)) & 0xffff0000u;
    r[i] = lo | hi;
  }
  return r;
}

// ---- max_pooling2d(2,2) on padded-NHWC bf16; one thread = 8 channels of one output pixel --------
__global__ __launch_bounds__(256) void maxpool_kernel(const __bf16* __restrict__ x, __bf16* __restrict__ y, int N,
                                                     int Ho, int Wo, int C) {
  const int c8 = C >> 3;
  const int64_t total = (int64_t)N * Ho * Wo * c8;
  const int Hi = Ho * 2, Wi = Wo * 2;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int cg = (int)(idx % c8);
    int64_t r = idx / c8;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho);
    const int n = (int)(r / Ho);
    const __bf16* src = x + (((int64_t)n * (Hi + 2) + (2 * oy + 1)) * (Wi + 2) + (2 * ox + 1)) * C + cg * 8;
    const int64_t rowp = (int64_t)(Wi + 2) * C;
    u32x4 v = bf16x8_max(*reinterpret_cast<const u32x4*>(src), *reinterpret_cast<const u32x4*>(src + C));
    v = bf16x8_max(v, *reinterpret_cast<const u32x4*>(src + rowp));
    v = bf16x8_max(v, *reinterpret_cast<const u32x4*>(src + rowp + C));
    *reinterpret_cast<u32x4*>(y + (((int64_t)n * (Ho + 2) + (oy + 1)) * (Wo + 2) + (ox + 1)) * C + cg * 8) = v;
  }
}

// ---- upscore_conv5 + add_score: y = residual + relu(bilinear_x2(x)) (simple_fcn.py:82-85) ------
// scale / shift (may be null): inference batch norm between the deconv and its relu (custom_layers.py:112-119)
__global__ __launch_bounds__(256) void upsample2x_kernel(const __bf16* __restrict__ x, const __bf16* __restrict__ res,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        __bf16* __restrict__ y, int N, int Hi, int Wi, int C,
                                                        int relu) {
  const int c8 = C >> 3;
  const int Ho = Hi * 2, Wo = Wi * 2;
  const int64_t total = (int64_t)N * Ho * Wo * c8;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int cg = (int)(idx % c8);
    int64_t r = idx / c8;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho);
    const int n = (int)(r / Ho);
    int iy1, ix1;
    float wy1, wy0, wx1, wx0;
    bilinear_taps<2>(oy, iy1, wy1, wy0);
    bilinear_taps<2>(ox, ix1, wx1, wx0);
    // padded coords: logical i -> i + 1; i0 = i1 - 1 >= -1 and i1 <= Hi are inside the padded buffer
    const __bf16* p00 = x + (((int64_t)n * (Hi + 2) + iy1) * (Wi + 2) + ix1) * C + cg * 8;  // (iy0, ix0)
    const int64_t rowp = (int64_t)(Wi + 2) * C;
    const u32x4 a00 = *reinterpret_cast<const u32x4*>(p00), a01 = *reinterpret_cast<const u32x4*>(p00 + C);
    const u32x4 a10 = *reinterpret_cast<const u32x4*>(p00 + rowp), a11 = *reinterpret_cast<const u32x4*>(p00 + rowp + C);
    const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
    u32x4 rv = u32x4{0u, 0u, 0u, 0u};
    const int64_t oidx = (((int64_t)n * (Ho + 2) + (oy + 1)) * (Wo + 2) + (ox + 1)) * C + cg * 8;
    if (res) rv = *reinterpret_cast<const u32x4*>(res + oidx);
    u32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int sh = h * 16;
        const float f00 = bf16_bits_to_f32((a00[i] >> sh) & 0xffffu), f01 = bf16_bits_to_f32((a01[i] >> sh) & 0xffffu);
        const float f10 = bf16_bits_to_f32((a10[i] >> sh) & 0xffffu), f11 = bf16_bits_to_f32((a11[i] >> sh) & 0xffffu);
        float u = f00 * w00 + f01 * w01 + f10 * w10 + f11 * w11;
        if (scale) u = u * scale[cg * 8 + i * 2 + h] + shift[cg * 8 + i * 2 + h];
        if (relu) u = fmaxf(u, 0.f);
        v[h] = u + bf16_bits_to_f32((rv[i] >> sh) & 0xffffu);
      }
      out[i] = pack_bf16x2(v[0], v[1]);
    }
    *reinterpret_cast<u32x4*>(y + oidx) = out;
  }
}

__global__ __launch_bounds__(256) void concat_kernel(const u32x4* __restrict__ a, const u32x4* __restrict__ b,
                                                    u32x4* __restrict__ y, int64_t pixels, int ca8, int cb8) {
  const int cy8 = ca8 + cb8;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < pixels * cy8; idx += (int64_t)gridDim.x * 256) {
    const int64_t p = idx / cy8;
    const int c = (int)(idx - p * cy8);
    y[idx] = c < ca8 ? a[p * ca8 + c] : b[p * cb8 + (c - ca8)];
  }
}

}  // namespace

extern "C" int xv_maxpool2x2_fwd(const xv_act* x, const xv_act* y, void* stream) {
  XV_REQUIRE_BF16(x, y);
  XV_CHECK_ARG(x && y && x->data && y->data);
  XV_CHECK_SHAPE(x->n > 0 && x->h > 0 && x->w > 0 && x->c > 0 && (x->c & 7) == 0 && (x->h & 1) == 0 && (x->w & 1) == 0);
  XV_CHECK_SHAPE(y->n == x->n && y->h == x->h / 2 && y->w == x->w / 2 && y->c == x->c);
  const int64_t total = (int64_t)y->n * y->h * y->w * (y->c >> 3);
  hipLaunchKernelGGL(maxpool_kernel, dim3(xv_grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const __bf16*)x->data,
                     (__bf16*)y->data, y->n, y->h, y->w, y->c);
  return xv_launch_status();
}

extern "C" int xv_upsample2x_affine_act_add(const xv_act* x, const float* scale, const float* shift,
                                           const xv_act* residual, const xv_act* y, int relu, void* stream) {
  XV_REQUIRE_BF16(x, residual, y);
  XV_CHECK_ARG(x && y && x->data && y->data);
  XV_CHECK_ARG((scale == nullptr) == (shift == nullptr));
  XV_CHECK_SHAPE(x->n > 0 && x->h > 0 && x->w > 0 && x->c > 0 && (x->c & 7) == 0);
  XV_CHECK_SHAPE(y->n == x->n && y->h == 2 * x->h && y->w == 2 * x->w && y->c == x->c);
  const __bf16* res = nullptr;
  if (residual && residual->data) {
    XV_CHECK_SHAPE(residual->n == y->n && residual->h == y->h && residual->w == y->w && residual->c == y->c);
    res = (const __bf16*)residual->data;
  }
  const int64_t total = (int64_t)y->n * y->h * y->w * (y->c >> 3);
  hipLaunchKernelGGL(upsample2x_kernel, dim3(xv_grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                     (const __bf16*)x->data, res, scale, shift, (__bf16*)y->data, x->n, x->h, x->w, x->c, relu);
  return xv_launch_status();
}

extern "C" int xv_upsample2x_affine_relu_add(const xv_act* x, const float* scale, const float* shift,
                                            const xv_act* residual, const xv_act* y, void* stream) {
  XV_REQUIRE_BF16(x, residual, y);
  return xv_upsample2x_affine_act_add(x, scale, shift, residual, y, 1, stream);
}

extern "C" int xv_upsample2x_relu_add(const xv_act* x, const xv_act* residual, const xv_act* y, void* stream) {
  XV_REQUIRE_BF16(x, residual, y);
  return xv_upsample2x_affine_relu_add(x, nullptr, nullptr, residual, y, stream);
}

// Depth-to-space behind the dense transposed convolution (xv_deconv_dense_fwd): z holds the s*s output phases of every
// input pixel side by side in its channels ([(py*s + px)*C + c]); y[n][qy*s + py][qx*s + px][c] = act(z * scale + shift)
// [+ residual].  One thread = 8 channels of one output pixel; for a fixed output row the s*C channels of an input pixel
// are contiguous, so reads and writes are both 16-byte coalesced.
__global__ __launch_bounds__(256) void depth_to_space_kernel(const __bf16* __restrict__ z, const __bf16* __restrict__ res,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            __bf16* __restrict__ y, int N, int Hi, int Wi, int C, int S,
                                                            int relu) {
  const int c8 = C >> 3;
  const int Ho = Hi * S, Wo = Wi * S;
  const int64_t total = (int64_t)N * Ho * Wo * c8;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int cg = (int)(idx % c8);
    int64_t r = idx / c8;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho);
    const int n = (int)(r / Ho);
    const int qy = oy / S, py = oy - qy * S, qx = ox / S, px = ox - qx * S;
    const u32x4 a = *reinterpret_cast<const u32x4*>(z + (((int64_t)n * (Hi + 2) + qy + 1) * (Wi + 2) + qx + 1) * ((int64_t)S * S * C) +
                                                    (int64_t)(py * S + px) * C + cg * 8);
    const int64_t yoff = (((int64_t)n * (Ho + 2) + oy + 1) * (Wo + 2) + ox + 1) * C + cg * 8;
    u32x4 rr = {0, 0, 0, 0};
    if (res != nullptr) rr = *reinterpret_cast<const u32x4*>(res + yoff);
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float lo = bf16_bits_to_f32(a[w] & 0xffffu), hi = __builtin_bit_cast(float, a[w] & 0xffff0000u);
      if (scale != nullptr) {
        lo = lo * scale[cg * 8 + 2 * w] + shift[cg * 8 + 2 * w];
        hi = hi * scale[cg * 8 + 2 * w + 1] + shift[cg * 8 + 2 * w + 1];
      }
      if (relu) {
        lo = fmaxf(lo, 0.f);
        hi = fmaxf(hi, 0.f);
      }
      lo += bf16_bits_to_f32(rr[w] & 0xffffu);
      hi += __builtin_bit_cast(float, rr[w] & 0xffff0000u);
      o[w] = pack_bf16x2(lo, hi);
    }
    *reinterpret_cast<u32x4*>(y + yoff) = o;
  }
}

int xv_launch_depth_to_space(const xv_act* z, const float* scale, const float* shift, const xv_act* residual, const xv_act* y,
                             int stride, int relu, hipStream_t stream) {
  const int64_t total = (int64_t)y->n * y->h * y->w * (y->c >> 3);
  hipLaunchKernelGGL(depth_to_space_kernel, dim3(xv_grid_for(total)), dim3(256), 0, stream, (const __bf16*)z->data,
                     residual && residual->data ? (const __bf16*)residual->data : nullptr, scale, shift, (__bf16*)y->data, z->n,
                     z->h, z->w, y->c, stride, relu);
  return xv_launch_status();
}

// tf.layers.dropout(x, rate, training=True) (simple_fcn.py:50-62,71-78,124-126: the MC-dropout sites of encoder /
// decoder): each element is kept with probability 1 - rate and scaled by 1 / (1 - rate), else zero.  Counter-based
// random bits: a 64-bit mix of (seed, element index) per element, so a mask depends only on the seed, not on the launch
// geometry.  Runs over the whole padded buffer (the zero border stays zero).  One thread = 8 channels.
__device__ __forceinline__ uint32_t xv_mix32(uint64_t z) {  // splitmix64 finaliser, upper 32 bits
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

// the eight channels idx * 8 .. idx * 8 + 7 of a map dropped with `seed` (idx: index of the 16-byte group within the map)
__device__ __forceinline__ u32x4 dropout8(u32x4 v, int64_t idx, uint32_t drop_below, float scale, uint64_t seed) {
  u32x4 o;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t r0 = xv_mix32(seed ^ (uint64_t)(idx * 8 + 2 * w) * 0xd1342543de82ef95ull);
    const uint32_t r1 = xv_mix32(seed ^ (uint64_t)(idx * 8 + 2 * w + 1) * 0xd1342543de82ef95ull);
    const float lo = r0 >= drop_below ? bf16_bits_to_f32(v[w] & 0xffffu) * scale : 0.f;
    const float hi = r1 >= drop_below ? __builtin_bit_cast(float, v[w] & 0xffff0000u) * scale : 0.f;
    o[w] = pack_bf16x2(lo, hi);
  }
  return o;
}

__global__ __launch_bounds__(256) void dropout_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y, int64_t total8,
                                                     uint32_t drop_below, float scale, uint64_t seed) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total8; idx += (int64_t)gridDim.x * 256)
    y[idx] = dropout8(x[idx], idx, drop_below, scale, seed);
}

// MC-dropout samples of one map: y holds `plain` + T slots of the N-image map x, slot-major.  plain = 1 (the variance fusion
// model): slot 0 is x itself, slot t = 1 .. T is x dropped with seed0 + (t - 1) * stride; plain = 0 (the Bayesian FCN: samples
// only): slot t = 0 .. T-1 is x dropped with seed0 + t * stride -- bit for bit what dropout_kernel writes for that seed: the
// hash takes the element's index WITHIN its slot.  blockIdx.y = slot - first_slot; the whole padded slot is written (its
// border is x's zero border).  In place (x == y, first_slot = plain): a plain slot is left as it is and every other slot is
// read from itself.
__global__ __launch_bounds__(256) void dropout_samples_kernel(const u32x4* x, u32x4* y, int64_t slot8, int first_slot, int plain,
                                                             uint32_t drop_below, float scale, uint64_t seed0, uint64_t stride) {
  const int slot = (int)blockIdx.y + first_slot;
  const u32x4* src = x == y ? y + slot * slot8 : x;
  u32x4* dst = y + slot * slot8;
  const uint64_t seed = seed0 + (uint64_t)(slot - plain) * stride;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < slot8; idx += (int64_t)gridDim.x * 256) {
    const u32x4 v = src[idx];
    dst[idx] = slot < plain ? v : dropout8(v, idx, drop_below, scale, seed);
  }
}

extern "C" int xv_dropout(const xv_act* x, const xv_act* y, float rate, uint64_t seed, void* stream) {
  XV_REQUIRE_BF16(x, y);
  XV_CHECK_ARG(x && y && x->data && y->data && rate >= 0.f && rate < 1.f);
  XV_CHECK_SHAPE(x->n == y->n && x->h == y->h && x->w == y->w && x->c == y->c && (x->c & 7) == 0);
  XV_CHECK_SHAPE(x->dtype == XV_BF16 && y->dtype == XV_BF16);
  const int64_t total8 = (int64_t)x->n * (x->h + 2) * (x->w + 2) * (x->c >> 3);
  const double thr = (double)rate * 4294967296.0;
  hipLaunchKernelGGL(dropout_kernel, dim3(xv_grid_for(total8)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)x->data,
                     (u32x4*)y->data, total8, (uint32_t)(thr > 4294967295.0 ? 4294967295.0 : thr), 1.f / (1.f - rate), seed);
  return xv_launch_status();
}

static uint32_t dropout_threshold(float rate) {
  const double thr = (double)rate * 4294967296.0;
  return (uint32_t)(thr > 4294967295.0 ? 4294967295.0 : thr);
}

extern "C" int xv_dropout_samples(const xv_act* x, const xv_act* y, int num_samples, float rate, uint64_t seed0,
                                  uint64_t stride, void* stream) {
  XV_REQUIRE_BF16(x, y);
  XV_CHECK_ARG(x && y && x->data && y->data && rate >= 0.f && rate < 1.f && num_samples >= 1 && num_samples <= 1024);
  XV_CHECK_SHAPE(x->n > 0 && (int64_t)y->n == (int64_t)x->n * (num_samples + 1) && x->h == y->h && x->w == y->w &&
                 x->c == y->c && (x->c & 7) == 0 && xv_dims_sane(y->n, y->h, y->w));
  const int64_t slot8 = (int64_t)x->n * (x->h + 2) * (x->w + 2) * (x->c >> 3);
  const char* xb = (const char*)x->data;
  const char* yb = (const char*)y->data;
  XV_CHECK_ARG(xb + slot8 * 16 <= yb || yb + (num_samples + 1) * slot8 * 16 <= xb);  // out of place: disjoint buffers
  hipLaunchKernelGGL(dropout_samples_kernel, dim3(xv_grid_for(slot8, 256, 2048), num_samples + 1), dim3(256), 0,
                     (hipStream_t)stream, (const u32x4*)x->data, (u32x4*)y->data, slot8, 0, 1, dropout_threshold(rate),
                     1.f / (1.f - rate), seed0, stride);
  return xv_launch_status();
}

extern "C" int xv_dropout_samples_inplace(const xv_act* y, int num_samples, float rate, uint64_t seed0, uint64_t stride,
                                          void* stream) {
  XV_REQUIRE_BF16(y);
  XV_CHECK_ARG(y && y->data && rate >= 0.f && rate < 1.f && num_samples >= 1 && num_samples <= 1024);
  XV_CHECK_SHAPE(y->n > 0 && y->n % (num_samples + 1) == 0 && (y->c & 7) == 0 && xv_dims_sane(y->n, y->h, y->w));
  const int64_t slot8 = (int64_t)(y->n / (num_samples + 1)) * (y->h + 2) * (y->w + 2) * (y->c >> 3);
  hipLaunchKernelGGL(dropout_samples_kernel, dim3(xv_grid_for(slot8, 256, 2048), num_samples), dim3(256), 0,
                     (hipStream_t)stream, (const u32x4*)y->data, (u32x4*)y->data, slot8, 1, 1, dropout_threshold(rate),
                     1.f / (1.f - rate), seed0, stride);
  return xv_launch_status();
}

// The sample-only forms (the Bayesian FCN computes T slots, not T + 1): y->n == num_samples x->n, slot t = xv_dropout(x, rate,
// seed0 + t stride); in place every slot of y is dropped.
extern "C" int xv_dropout_samples_only(const xv_act* x, const xv_act* y, int num_samples, float rate, uint64_t seed0,
                                       uint64_t stride, void* stream) {
  XV_REQUIRE_BF16(x, y);
  XV_CHECK_ARG(x && y && x->data && y->data && rate >= 0.f && rate < 1.f && num_samples >= 1 && num_samples <= 1024);
  XV_CHECK_SHAPE(x->n > 0 && (int64_t)y->n == (int64_t)x->n * num_samples && x->h == y->h && x->w == y->w && x->c == y->c &&
                 (x->c & 7) == 0 && xv_dims_sane(y->n, y->h, y->w));
  const int64_t slot8 = (int64_t)x->n * (x->h + 2) * (x->w + 2) * (x->c >> 3);
  const char* xb = (const char*)x->data;
  const char* yb = (const char*)y->data;
  XV_CHECK_ARG(xb + slot8 * 16 <= yb || yb + num_samples * slot8 * 16 <= xb);  // out of place: disjoint buffers
  hipLaunchKernelGGL(dropout_samples_kernel, dim3(xv_grid_for(slot8, 256, 2048), num_samples), dim3(256), 0, (hipStream_t)stream,
                     (const u32x4*)x->data, (u32x4*)y->data, slot8, 0, 0, dropout_threshold(rate), 1.f / (1.f - rate), seed0,
                     stride);
  return xv_launch_status();
}

extern "C" int xv_dropout_samples_only_inplace(const xv_act* y, int num_samples, float rate, uint64_t seed0, uint64_t stride,
                                               void* stream) {
  XV_REQUIRE_BF16(y);
  XV_CHECK_ARG(y && y->data && rate >= 0.f && rate < 1.f && num_samples >= 1 && num_samples <= 1024);
  XV_CHECK_SHAPE(y->n > 0 && y->n % num_samples == 0 && (y->c & 7) == 0 && xv_dims_sane(y->n, y->h, y->w));
  const int64_t slot8 = (int64_t)(y->n / num_samples) * (y->h + 2) * (y->w + 2) * (y->c >> 3);
  hipLaunchKernelGGL(dropout_samples_kernel, dim3(xv_grid_for(slot8, 256, 2048), num_samples), dim3(256), 0, (hipStream_t)stream,
                     (const u32x4*)y->data, (u32x4*)y->data, slot8, 0, 0, dropout_threshold(rate), 1.f / (1.f - rate), seed0,
                     stride);
  return xv_launch_status();
}

// Dropout of the network INPUT, whole pixels at a time (uncertainty_dirichlet_mix.py:106-116: tf.layers.dropout with
// noise_shape [N, H, W, 1]): ONE draw per (image, row, column), shared by the pixel's channels; a kept pixel is scaled by
// 1 / (1 - rate) in fp32.  x is the dense fp32 NHWC input; y holds `plain` + T slots of it, slot-major: slot 0 a copy of x when
// plain, sample t = 0 .. T-1 dropped with seed0 + t * stride.  The bits are xv_mix32 of (seed, index of the PIXEL within its
// slot), as dropout8 mixes (seed, element index): a mask depends on nothing else -- not on the launch geometry, the channel
// count or how the samples are dealt out over calls.  One thread per ELEMENT (coalesced 4-byte accesses; the pixel's hash is
// recomputed per channel, which a streaming copy of three channels does not notice); blockIdx.y = slot.
__global__ __launch_bounds__(256) void pixel_dropout_kernel(const float* __restrict__ x, float* __restrict__ y, uint32_t slot_elems,
                                                           uint32_t cin, int plain, uint32_t drop_below, float scale,
                                                           uint64_t seed0, uint64_t stride) {
  const int slot = (int)blockIdx.y;
  float* dst = y + (int64_t)slot * slot_elems;
  const uint64_t seed = seed0 + (uint64_t)(slot - plain) * stride;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < slot_elems; i += gridDim.x * 256u) {
    const float v = x[i];
    const uint32_t r = xv_mix32(seed ^ (uint64_t)(i / cin) * 0xd1342543de82ef95ull);
    dst[i] = slot < plain ? v : (r >= drop_below ? v * scale : 0.f);
  }
}

extern "C" int xv_dropout_pixels_samples(const float* x, int n, int h, int w, int cin, float* y, int num_samples, int plain,
                                         float rate, uint64_t seed0, uint64_t stride, void* stream) {
  XV_CHECK_ARG(x && y && rate >= 0.f && rate < 1.f && num_samples >= 1 && num_samples <= 1024 && (plain == 0 || plain == 1));
  XV_CHECK_SHAPE(n > 0 && h > 0 && w > 0 && cin > 0 && (int64_t)n * h * w * cin < ((int64_t)1 << 31) - 256 * 2048);
  const int64_t slot = (int64_t)n * h * w * cin, slots = num_samples + plain;
  const char* xb = (const char*)x;
  const char* yb = (const char*)y;
  XV_CHECK_ARG(xb + slot * 4 <= yb || yb + slots * slot * 4 <= xb);  // out of place: disjoint buffers
  hipLaunchKernelGGL(pixel_dropout_kernel, dim3(xv_grid_for(slot, 256, 2048), (unsigned)slots), dim3(256), 0, (hipStream_t)stream, x,
                     y, (uint32_t)slot, (uint32_t)cin, plain, dropout_threshold(rate), 1.f / (1.f - rate), seed0, stride);
  return xv_launch_status();
}

// y[..., :Ca] = a, y[..., Ca:] = b over the whole padded buffers (tf.concat(axis=3), fusion_fcn.py:27-28)
extern "C" int xv_concat_channels(const xv_act* a, const xv_act* b, const xv_act* y, void* stream) {
  XV_REQUIRE_BF16(a, b, y);
  XV_CHECK_ARG(a && b && y && a->data && b->data && y->data);
  XV_CHECK_SHAPE(a->n == b->n && a->h == b->h && a->w == b->w && y->n == a->n && y->h == a->h && y->w == a->w);
  XV_CHECK_SHAPE(y->c == a->c + b->c && (a->c & 7) == 0 && (b->c & 7) == 0);
  const int64_t total = (int64_t)y->n * (y->h + 2) * (y->w + 2) * (y->c >> 3);
  hipLaunchKernelGGL(concat_kernel, dim3(xv_grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)a->data,
                     (const u32x4*)b->data, (u32x4*)y->data, (int64_t)y->n * (y->h + 2) * (y->w + 2), a->c >> 3,
                     b->c >> 3);
  return xv_launch_status();
}
