// Shared device/host helpers for libxview_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/xview_hip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

#define XV_CHECK_ARG(cond) \
  do {                     \
    if (!(cond)) return XV_EINVAL; \
  } while (0)
#define XV_CHECK_SHAPE(cond) \
  do {                       \
    if (!(cond)) return XV_ESHAPE; \
  } while (0)

// bf16-only entry points (everything except the forward convolutions, which read / write e4m3 maps too): an XV_FP8
// descriptor handed to them would be reinterpreted as bf16 -- garbage and reads past the end of a map of half the bytes.
// Null descriptors (optional arguments) pass; the entry point's own argument checks deal with them.
static inline bool xv_all_bf16(std::initializer_list<const xv_act*> acts) {
  for (const xv_act* a : acts)
    if (a != nullptr && a->dtype != XV_BF16) return false;
  return true;
}
#define XV_REQUIRE_BF16(...)                               \
  do {                                                     \
    if (!xv_all_bf16({__VA_ARGS__})) return XV_EINVAL;     \
  } while (0)

static inline int xv_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? XV_OK : (int)e;
}

// blocks of a grid-stride launch over `total` items: one block per `per_block` items, at least one, at most `cap`
static inline int xv_grid_for(int64_t total, int per_block = 256, int cap = 8192) {
  int64_t g = (total + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// Launchers of kernels templated on the padded class count CM (a multiple of 4, at most 32): CALL(CM) for the smallest CM that
// holds C_ classes.  CALL is a statement or a block.
#define XV_CM_SWITCH(C_, CALL) \
  switch (((C_) + 3) / 4) {    \
    case 1: CALL(4); break;    \
    case 2: CALL(8); break;    \
    case 3: CALL(12); break;   \
    case 4: CALL(16); break;   \
    case 5: CALL(20); break;   \
    case 6: CALL(24); break;   \
    case 7: CALL(28); break;   \
    default: CALL(32); break;  \
  }

// Per-device caches (one process normally drives one GPU, but nothing here may depend on it): up to XV_MAX_DEVICES devices
// of one process; an out-of-range device index falls back to querying every time.
#define XV_MAX_DEVICES 16
static inline int xv_current_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess ? dev : 0;
}

// CU count of the current device (cached per device; 256 on MI355X) -- sizes persistent grids.
static inline int xv_num_cus() {
  static int cus[XV_MAX_DEVICES] = {0};
  const int dev = xv_current_device();
  if (dev >= 0 && dev < XV_MAX_DEVICES && cus[dev] > 0) return cus[dev];
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  if (dev >= 0 && dev < XV_MAX_DEVICES) cus[dev] = n;
  return n;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device and per kernel: `done` is the kernel's own flag array
static inline hipError_t xv_allow_dynamic_lds(const void* kernel, int bytes, bool (&done)[XV_MAX_DEVICES],
                                              bool from_offset_0 = true) {
  const int dev = xv_current_device();
  if (dev >= 0 && dev < XV_MAX_DEVICES && done[dev]) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess && from_offset_0) {
    // The conv kernels behind this helper address their dynamic LDS from offset 0 (LDS-DMA destinations in M0, ds_read offsets in
    // assembly).  A static LDS object in front of it -- the compiler promotes an alloca into LDS when a struct does not stay
    // in registers: round 4, a bool member in the tile record -- would sit on top of the first operand buffer: refuse to launch.
    hipFuncAttributes attr;
    e = hipFuncGetAttributes(&attr, kernel);
    if (e == hipSuccess && attr.sharedSizeBytes != 0) e = hipErrorInvalidConfiguration;
  }
  if (e == hipSuccess && dev >= 0 && dev < XV_MAX_DEVICES) done[dev] = true;
  return e;
}

// A map this library can address at all: positive dimensions, sides below 2^24, fewer than 2^31 padded rows and 2^36
// padded pixels (64 G pixels: beyond any 288 GB buffer).  The size calculators return 0 and the choosers XV_ESHAPE past it, so that their
// 64-bit arithmetic cannot overflow (tools/asan_host_check.py fuzzes them under UBSan).
static inline bool xv_dims_sane(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0 || h >= (1 << 24) || w >= (1 << 24)) return false;
  const int64_t rows = (int64_t)n * ((int64_t)h + 2);
  return rows < ((int64_t)1 << 31) && rows * ((int64_t)w + 2) < ((int64_t)1 << 36);
}

// ln C as the uncertainty kernels divide by it (custom_layers.py:251-256 normalises the entropy to [0, 1]): one host value for
// the head and the stand-alone reduction
static inline float xv_ln_classes(int num_classes) { return (float)log((double)num_classes); }

// padded-NHWC geometry helpers
__host__ __device__ static inline int64_t xv_row_pitch(int w, int c) { return (int64_t)(w + 2) * c; }
__host__ __device__ static inline int64_t xv_img_pitch(int h, int w, int c) {
  return (int64_t)(h + 2) * (w + 2) * c;
}

// 16-byte-slot swizzle shared by the weight packer and the conv kernels: slot s of the 128-byte
// LDS row of weight row / patch column `row` lives at slot s ^ (row & 6).  Two consecutive 128-B
// rows fill one 256-B LDS bank row; a ds_read_b128 is served in 16-lane groups that, for the
// 16x16x32 MFMA fragment map, hold 16 consecutive rows with two adjacent logical slots
// ({0-3,12-15} slot a, {4-11} slot a+1).  An exhaustive search over GF(2)-linear maps of the row
// index (tools/lds_swizzle_search.py) shows `row & 6` is conflict-free for EVERY starting row, i.e.
// for all three horizontal taps of a 3x3 conv; the earlier (row>>1)&7 was 2-way for 3 of 4 starts.
// For activation patches `row` is the pixel's COLUMN inside the patch (the patch pitch is even, so
// bank-row parity is preserved), which makes the swizzle independent of the patch row and lets
// every fragment read be base-register + immediate.
__host__ __device__ static inline int xv_swz(int row, int slot) { return slot ^ (row & 6); }

// 64-byte rows (generation-2 conv kernel): slot s of row `row` lives at s ^ ((row >> 1) & 2)
__host__ __device__ static inline int xv_swz32(int row, int slot) { return slot ^ ((row >> 1) & 2); }

// four fp32 -> four OCP e4m3 bytes (round-to-nearest-even) of value * mul, saturating at the largest finite e4m3 (the
// conversion's own overflow behaviour depends on a mode bit, so the clamp is explicit)
__device__ static inline uint32_t xv_pack_fp8x4(float v0, float v1, float v2, float v3, float mul) {
  const float a = __builtin_amdgcn_fmed3f(v0 * mul, -448.f, 448.f);
  const float b = __builtin_amdgcn_fmed3f(v1 * mul, -448.f, 448.f);
  const float c = __builtin_amdgcn_fmed3f(v2 * mul, -448.f, 448.f);
  const float d = __builtin_amdgcn_fmed3f(v3 * mul, -448.f, 448.f);
  int p = 0;
  p = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, p, false);
  p = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, p, true);
  return (uint32_t)p;
}

__device__ static inline uint32_t pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
  bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}

__device__ static inline float bf16_bits_to_f32(uint32_t bits16) {
  return __builtin_bit_cast(float, bits16 << 16);
}

// the two bf16 halves of a packed word as fp32
__device__ static __forceinline__ float bf_lo(uint32_t v) { return __builtin_bit_cast(float, v << 16); }
__device__ static __forceinline__ float bf_hi(uint32_t v) { return __builtin_bit_cast(float, v & 0xffff0000u); }

// Bilinear transposed-conv taps ([TF1] conv2d_transpose 'same': out o receives in i through kernel
// index p with o = i*S + p - S/2, k = 2S): sources i1 = (o + S/2) / S with p1 = (o + S/2) % S and
// i0 = i1 - 1 with p0 = p1 + S; 1-D weight w1[p] = 1 - |p/S - (2S-1-S%2)/(2S)| (custom_layers.py:15-21).
// Out-of-range sources fall on the zero border of the padded layout and contribute exactly 0.
template <int S>
__device__ static inline void bilinear_taps(int o, int& i1, float& w_i1, float& w_i0) {
#pragma clang fp contract(on)
  const int t = o + S / 2;
  i1 = t / S;
  const int p1 = t - i1 * S;
  constexpr float center = (2.f * S - 1.f - (S % 2)) / (2.f * S);
  w_i1 = 1.f - fabsf((float)p1 / S - center);
  w_i0 = 1.f - fabsf((float)(p1 + S) / S - center);
}

// ---- exact three-way bf16 split of fp32 MFMA operands (conv_first.hip, conv_first_fused.hip, batchnorm.hip) ------------------
// The k-slot map of conv1_1 on 16 x 16 x 32 bf16 MFMAs (K = 9 CIN <= 27 fits one MFMA): k-group g (8 values, lanes 16 g ..
// 16 g + 15) holds image row dy = g, columns dx = 0..2 x CIN channels in memory order (8 of its 9 values for CIN = 3); the
// three leftover values (dx = 2, ci = 2 of each row) form k-group 3, whose first spare slot carries the bias.
template <int CIN>
__device__ static __forceinline__ bool first_k_map(int g, int e, int& dy, int& dx, int& ci) {
  if (CIN == 3) {
    if (g < 3) {
      dy = g, dx = e / 3, ci = e % 3;
      return true;
    }
    dy = e, dx = 2, ci = 2;
    return e < 3;
  }
  dy = g, dx = e, ci = 0;  // CIN == 1
  return g < 3 && e < 3;
}

// v = h + m + l exactly, each term a bf16 (returned as fp32 bit patterns with zero low halves): truncation keeps the
// top 8 significant bits, the remainder of a 24-bit significand has at most 16, then at most 8
__device__ static __forceinline__ void split3_bf16(float v, uint32_t& h, uint32_t& m, uint32_t& l) {
  h = __builtin_bit_cast(uint32_t, v) & 0xffff0000u;
  const float r1 = v - __builtin_bit_cast(float, h);  // exact
  m = __builtin_bit_cast(uint32_t, r1) & 0xffff0000u;
  l = __builtin_bit_cast(uint32_t, r1 - __builtin_bit_cast(float, m));  // exact, fits 8 bits
}
__device__ static __forceinline__ uint32_t hi16_pair(uint32_t a, uint32_t b) {  // (a >> 16) | (b & 0xffff0000): v_perm_b32
  return __builtin_amdgcn_perm(b, a, 0x07060302u);
}
__device__ static __forceinline__ void split3_bf16x8(const float (&v)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
  uint32_t hh[8], mm[8], ll[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) split3_bf16(v[e], hh[e], mm[e], ll[e]);
  h = __builtin_bit_cast(bf16x8, u32x4{hi16_pair(hh[0], hh[1]), hi16_pair(hh[2], hh[3]), hi16_pair(hh[4], hh[5]), hi16_pair(hh[6], hh[7])});
  m = __builtin_bit_cast(bf16x8, u32x4{hi16_pair(mm[0], mm[1]), hi16_pair(mm[2], mm[3]), hi16_pair(mm[4], mm[5]), hi16_pair(mm[6], mm[7])});
  l = __builtin_bit_cast(bf16x8, u32x4{hi16_pair(ll[0], ll[1]), hi16_pair(ll[2], ll[3]), hi16_pair(ll[4], ll[5]), hi16_pair(ll[6], ll[7])});
}

// Output-side helpers shared by the MFMA conv kernels (a lane holds 4 consecutive output channels of one pixel for
// each of the four 16-channel blocks).
__device__ static __forceinline__ void xv_pair16(const u32x2 a, const u32x2 b, u32x4& out) {
  // lanes of row r (= lane >> 4) hold channel groups r*4 of `a` (block j) and `b` (block j+1); after the swap a
  // lane holds 8 consecutive channels: rows 0..3 -> channel offsets 0, 16, 8, 24 of the 32-channel pair
  const auto s0 = __builtin_amdgcn_permlane16_swap(a.x, b.x, false, false);
  const auto s1 = __builtin_amdgcn_permlane16_swap(a.y, b.y, false, false);
  out = u32x4{s0[0], s1[0], s0[1], s1[1]};
}

// relu and 2x2 max on PACKED bf16 pairs: a non-negative bf16 orders like its bit pattern as a signed 16-bit
// integer and every negative one (sign bit) is a negative integer, so relu is v_pk_max_i16 against 0 and, after
// it, so is the max-pool -- two values per instruction and none of the NaN-quieting v_max_f32 x,x,x that fmaxf
// costs under IEEE mode.  Rounding to bf16 is monotone, so pooling after rounding equals rounding after pooling.
__device__ static __forceinline__ uint32_t pk_max_i16(uint32_t a, uint32_t b) {
  typedef short s16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}

// The per-pixel softmax / log-probability arithmetic of the heads (tf.nn.softmax, Dirichlet.log_prob: basic_fusion_model.py:
// 21-22, dirichlet_mix.py:23-36) on the transcendental unit: v_exp_f32 / v_log_f32 / v_rcp_f32 (about 1 ulp each, denormal
// inputs / results flushed) in place of the correctly rounded library forms (10-15 instructions each; an IEEE division is ten).
// xv_fast_exp(x) = exp2(x * log2 e): the rounding of the product is amplified by |x|, so its relative error GROWS as
// ~|x| * 6e-8 (6e-7 at x = -10, 5e-6 at x = -80) -- terms that small are below fp32 resolution of the softmax sum they
// enter.  Probabilities, Dirichlet log-probabilities and the training loss are therefore NOT correctly rounded libm
// results (numerics notes); the accuracy tests bound what that costs.  24 logs, 24 exps and 48 divisions
// per pixel made the fused Dirichlet head 10x slower than its 288 FMAs.  Every kernel that must agree
// bit for bit with another one (fused head <-> head + fusion kernels) uses the same helper.
__device__ static __forceinline__ float xv_fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ static __forceinline__ float xv_fast_log(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }
__device__ static __forceinline__ float xv_fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// Certainty-weighted fusion of the MC-dropout model (variance_mix.py:7-15): fused[k] = sum_e p_e[k] c_e / sum_e c_e with the
// certainty c_e = 1 / (1e-20 + var_e).  The variance head (heads.hip) and xv_variance_fuse (fusion.hip) both run these two
// functions, experts in the same order, so their labels agree bit for bit.  Contraction is off inside them: a caller's
// product must not be fused into `1e-20 + var` in one kernel and not in the other.
template <int CM>
__device__ static __forceinline__ void xv_variance_fuse_add(float (&acc)[CM], float& csum, const float (&p)[CM], float var,
                                                             bool first) {
#pragma clang fp contract(off)
  const float c = 1.f / (1e-20f + var);
#pragma unroll
  for (int k = 0; k < CM; ++k) acc[k] = first ? p[k] * c : __builtin_fmaf(p[k], c, acc[k]);
  csum = first ? c : csum + c;
}

// acc <- the fused score; returns its argmax over the first C classes (lowest index on ties, tf.argmax)
template <int CM>
__device__ static __forceinline__ int xv_variance_fuse_finish(float (&acc)[CM], float csum, int C) {
#pragma clang fp contract(off)
  float best = 0.f;
  int bi = 0;
#pragma unroll
  for (int k = 0; k < CM; ++k) {
    acc[k] = acc[k] / csum;
    if (k < C && (k == 0 || acc[k] > best)) {
      best = acc[k];
      bi = k;
    }
  }
  return bi;
}

// Per-pixel moments of the MC-dropout Bayesian FCN (bayesian_fcn.py:48-57 sampling_uncertainty, custom_layers.py:251-256
// entropy) over T samples p_t of a pixel's class probabilities, ONE pass over the samples (each is seen once), Welford's
// running form:
//   first:  mean = p_1, m2 = 0, ce = H(p_1)
//   add:    d = p_t - mean; mean += d * (1 / t); m2 = fma(d, p_t - mean, m2); ce += H(p_t)       (t = 2 .. T, in this order)
//   finish: variance = (sum_c max(m2_c, 0)) / T; entropy = H(mean) / ln C; cond_entropy = ce / T / ln C; returns argmax_c mean
//           (lowest index on ties)
// with H(p) = -sum_c p_c ln(clip(p_c, 1e-10, 1)), classes in ascending order, xv_fast_log after the clip (no denormal reaches
// it).  Identical samples give d = 0 at every step: variance exactly 0 and mean exactly p_1 (the mean of T equal fp32 values,
// summed and scaled, need not be that value); a negative rounding residue of m2 is clamped per class, so variance >= 0.
// T = 1: mean = p_1, so entropy and cond_entropy are the same expression on the same bits.  Two rows of state (mean, m2) where
// the shifted sums of variance_head_kernel take three: at 16 classes that is what keeps the head at four waves per SIMD.
// The head (heads.hip, mc_uncertainty_head_kernel) and xv_sampling_uncertainty (fusion.hip) both run these functions, so
// equal p_t give equal bits; contraction is off inside them so that neither caller's context decides where an fma forms.
// Lanes k >= C are ignored.
template <int CM>
__device__ static __forceinline__ float xv_entropy_sum(const float (&p)[CM], int C) {
#pragma clang fp contract(off)
  float h = 0.f;
#pragma unroll
  for (int k = 0; k < CM; ++k)
    if (k < C) h -= p[k] * xv_fast_log(fminf(fmaxf(p[k], 1e-10f), 1.f));
  return h;
}

template <int CM>
__device__ static __forceinline__ void xv_mc_first(float (&mean)[CM], float (&m2)[CM], float& ce, const float (&p)[CM], int C,
                                                    bool want_ce) {
#pragma unroll
  for (int k = 0; k < CM; ++k) mean[k] = p[k], m2[k] = 0.f;
  ce = want_ce ? xv_entropy_sum<CM>(p, C) : 0.f;
}

// sample number t (1-based, t >= 2)
template <int CM>
__device__ static __forceinline__ void xv_mc_add(float (&mean)[CM], float (&m2)[CM], float& ce, const float (&p)[CM], int t,
                                                  int C, bool want_ce, bool want_var) {
#pragma clang fp contract(off)
  const float inv_t = 1.f / (float)t;
#pragma unroll
  for (int k = 0; k < CM; ++k) {
    const float d = p[k] - mean[k];
    mean[k] = mean[k] + d * inv_t;
    if (want_var) m2[k] = __builtin_fmaf(d, p[k] - mean[k], m2[k]);
  }
  if (want_ce) ce = ce + xv_entropy_sum<CM>(p, C);
}

// ln_c = (float)ln C from the host (xv_ln_classes)
template <int CM>
__device__ static __forceinline__ int xv_mc_finish(const float (&mean)[CM], const float (&m2)[CM], float ce, int T, int C,
                                                    float ln_c, bool want_ent, float& entropy, float& cond_entropy,
                                                    float& variance) {
#pragma clang fp contract(off)
  const float inv_t = 1.f / (float)T;
  float var = 0.f, best = 0.f;
  int bi = 0;
#pragma unroll
  for (int k = 0; k < CM; ++k)
    if (k < C) {
      var = var + fmaxf(m2[k], 0.f);
      if (k == 0 || mean[k] > best) best = mean[k], bi = k;
    }
  variance = var * inv_t;
  entropy = want_ent ? xv_entropy_sum<CM>(mean, C) / ln_c : 0.f;
  cond_entropy = ce * inv_t / ln_c;
  return bi;
}

// Uncertainty-weighted Dirichlet fusion (uncertainty_dirichlet_mix.py:18-52): per expert and pixel the fitted parameters are
// softened towards the standard ones (ones plus the identity) by mix = mean_c variance / max variance,
//   alpha[j][c] = A[j][c] (1 - mix) + mix (1 + delta_jc),
//   ll[c] = sum_j (alpha[j][c] - 1) log(1e-20 + p[j] / sum p) + lgamma(sum_j alpha[j][c]) - sum_j lgamma(alpha[j][c]),
// and score[c] = sum_e ll_e[c] + logprior[c].  The parameters differ per pixel, so the C^2 + C lgamma per expert are taken here
// (ocml's lgammaf; its call sites stay ROLLED -- one copy per expert instead of C^2 -- while the dot products over j unroll on
// statically indexed registers).  `A` is one expert's table in LDS, TRANSPOSED and padded with zeros: A[c * CM + j] = A[j][c];
// `cs[c]` = sum_j A[j][c] rounded once from double: sum_j alpha[j][c] = cs[c] (1 - mix) + mix (C + 1) is linear in mix.
// mix = 1 gives alpha = 1 + delta_jc exactly, whatever A holds; mix = 0 gives alpha = A exactly.  Renormalisation and logarithm
// are those of dirichlet_fuse_kernel (xv_fast_rcp, xv_fast_log).  The fusion head (heads.hip) and
// xv_uncertainty_dirichlet_fuse (fusion.hip) both run these functions: equal p, mvar and vmax give equal bits, for any CM >= C
// (padding adds exact zeros); contraction is off inside them.  max variance 0 (identical samples everywhere; the reference
// divides 0 / 0 there) gives mix = 0, the plain Dirichlet fusion.
__device__ static __forceinline__ float xv_udm_mix(float mvar, float vmax) {
#pragma clang fp contract(off)
  return vmax > 0.f ? fminf(mvar / vmax, 1.f) : 0.f;
}

__device__ static __forceinline__ float xv_udm_alpha(float a, float om, float mix, bool diag) {
  return __builtin_fmaf(a, om, diag ? mix + mix : mix);
}

template <int CM>
__device__ static __forceinline__ void xv_udm_add(float (&total)[CM], const float (&p)[CM], float mix, const float* A,
                                                   const float* cs, int C, bool first) {
#pragma clang fp contract(off)
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < CM; ++k) sum = sum + p[k];
  const float rs = xv_fast_rcp(sum);
  float lx[CM];
#pragma unroll
  for (int k = 0; k < CM; ++k) lx[k] = k < C ? xv_fast_log(__builtin_fmaf(p[k], rs, 1e-20f)) : 0.f;
  const float om = 1.f - mix;
  const float top = mix * (float)(C + 1);
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    const float* row = A + c * CM;
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < CM; ++j) dot = __builtin_fmaf(xv_udm_alpha(row[j], om, mix, j == c) - 1.f, lx[j], dot);
    float lg = 0.f;
#pragma unroll 1
    for (int j = 0; j < C; ++j) lg = lg + lgammaf(xv_udm_alpha(row[j], om, mix, j == c));
    const float L = (dot + lgammaf(__builtin_fmaf(cs[c], om, top))) - lg;
#pragma unroll
    for (int cc = 0; cc < CM; ++cc)           // static register indexing: a select, not total[c] with a run-time c
      if (cc == c) total[cc] = first ? L : total[cc] + L;
  }
}

// total <- the fused score; returns its argmax over the first C classes (lowest index on ties, tf.argmax)
template <int CM>
__device__ static __forceinline__ int xv_udm_finish(float (&total)[CM], const float* lp, int C) {
#pragma clang fp contract(off)
  float best = 0.f;
  int bi = 0;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {
      total[c] = total[c] + lp[c];
      if (c == 0 || total[c] > best) best = total[c], bi = c;
    }
  return bi;
}

// One expert's [C][C] parameters (A[j][c], row-major over j) into the LDS table xv_udm_add reads: nthreads threads of a
// workgroup; the caller synchronises afterwards.
template <int CM>
__device__ static __forceinline__ void xv_udm_stage(float* tab, float* cs, const float* __restrict__ A_g, int C, int tid,
                                                     int nthreads) {
  for (int i = tid; i < C * CM; i += nthreads) {
    const int j = i % CM, c = i / CM;
    tab[i] = j < C ? A_g[j * C + c] : 0.f;
  }
  for (int c = tid; c < CM; c += nthreads) {
    double s = 0.0;
    if (c < C)
      for (int j = 0; j < C; ++j) s += (double)A_g[j * C + c];
    cs[c] = (float)s;
  }
}

// A workgroup's maximum of non-negative floats (they order like their bit patterns) into *dst with ONE atomic: registers,
// then the wave (DPP-free shuffles), then LDS (`red`: one word per wave).  Every thread of the workgroup calls it.
__device__ static __forceinline__ void xv_block_max_nonneg(float v, uint32_t* red, uint32_t* dst) {
  uint32_t b = __builtin_bit_cast(uint32_t, v);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)b, off, 64);
    b = o > b ? o : b;
  }
  const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < nw; ++i) b = red[i] > b ? red[i] : b;
    if (b) atomicMax(dst, b);
  }
}

// ---- uncertainty benchmarks (uncertainty_model.py; xv_uncertainty_stats in fusion.hip, xv_mc_uncertainty_score_fwd in
// heads.hip) -------------------------------------------------------------------------------------------------------------
// Histogram bin of a metric value from its BIT PATTERN (non-negative floats order like their bits, as xv_block_max_nonneg
// uses): M mantissa bits and `octaves` binades below 2 give octaves << M log-spaced bins of 2^-M relative width;
// key = (bits >> (23 - M)) - ((128 - octaves) << M) clamped to [0, bins - 1].  v <= 0 (and -0.0) -> bin 0, NaN -> the top bin
// (as every value >= 2 and +inf).  An exact function of the bits: uncertainty_model.bin_index is the same expression in numpy.
__device__ static __forceinline__ int xv_unc_bin(float v, int M, int octaves) {
  const int top = (octaves << M) - 1;
  if (v != v) return top;
  if (!(v > 0.f)) return 0;
  const int key = (int)(__builtin_bit_cast(uint32_t, v) >> (23 - M)) - ((128 - octaves) << M);
  return key < 0 ? 0 : (key > top ? top : key);
}

// One pixel's NLL term of the benchmarks, -ln(clip(p, 1e-10, 1)) with xv_fast_log after the clip (the logarithm of
// xv_entropy_sum), as a double for the double sums.
__device__ static __forceinline__ double xv_unc_nll_term(float p) {
  return -(double)xv_fast_log(fminf(fmaxf(p, 1e-10f), 1.f));
}

// The replicated LDS tables of both kernels, index = cell * rep + copy: nll double [C][rep], cnt u64 [C][rep], then hist u32
// [nhist][2][bins][rep].  Zeroed by the workgroup; at the end every cell's copies are summed and each non-zero cell costs ONE
// global atomic.  `ncls` = 0: no NLL tables.
__device__ static __forceinline__ void xv_unc_tables_zero(double* nll_s, int ncls, uint32_t* hist_s, int hcells, int rep) {
  for (int i = threadIdx.x; i < 2 * ncls * rep; i += blockDim.x) nll_s[i] = 0.0;  // (0.0 and 0ull share their bits)
  for (int i = threadIdx.x; i < hcells * rep; i += blockDim.x) hist_s[i] = 0u;
}

__device__ static __forceinline__ void xv_unc_tables_flush(const double* nll_s, int ncls, const uint32_t* hist_s, int hcells, int rep,
                                                           unsigned long long* __restrict__ hist, double* __restrict__ nll,
                                                           unsigned long long* __restrict__ counts) {
  const unsigned long long* cnt_s = reinterpret_cast<const unsigned long long*>(nll_s + ncls * rep);
  for (int i = threadIdx.x; i < hcells; i += blockDim.x) {
    unsigned long long a = 0ull;
    for (int r = 0; r < rep; ++r) a += hist_s[i * rep + r];
    if (a) atomicAdd(&hist[i], a);
  }
  for (int i = threadIdx.x; i < ncls; i += blockDim.x) {
    double s = 0.0;
    unsigned long long a = 0ull;
    for (int r = 0; r < rep; ++r) s += nll_s[i * rep + r], a += cnt_s[i * rep + r];
    if (a) {
      atomicAdd(&nll[i], s);
      atomicAdd(&counts[i], a);
    }
  }
}

// Order-preserving map of packed bf16 bit patterns onto signed 16-bit integers (an involution: negative values have their
// magnitude bits flipped), for a 2x2 max on packed pairs WITHOUT a preceding relu.
__device__ static __forceinline__ uint32_t pk_ord_bf16(uint32_t x) {
  typedef short s16x2 __attribute__((ext_vector_type(2)));
  const s16x2 v = __builtin_bit_cast(s16x2, x);
  const s16x2 m = (v >> 15) & (short)0x7fff;
  return __builtin_bit_cast(uint32_t, v ^ m);
}

// value of lane ^ 1 (DPP quad_perm [1,0,3,2]) of a packed register
__device__ static __forceinline__ uint32_t pk_dpp_swap1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);
}

// ---- diagnostic build only (-DXV_CLOCK_STAMP: `make stamp` -> tools/build/libxview_hip_stamp.so, read by tools/conv_clock.py;
// never in the shipped library) --------------------------------------------------------------------------------------------
// The clock the chip holds inside a conv kernel's item loop = delta s_memtime (shader cycles) / delta s_memrealtime (a
// constant 100 MHz counter) x 100 MHz, stamped ONCE around the loop by every workgroup (MI355X_MICROARCH.md, 'DVFS
// give-back' item 6).  The four values go to a buffer of their own after the loop; nothing is computed from them.
#ifdef XV_CLOCK_STAMP
#define XV_CLK_SLOTS 2048
#define XV_CLK_BEGIN()                                              \
  const unsigned long long clk_m0 = __builtin_amdgcn_s_memtime();   \
  const unsigned long long clk_r0 = __builtin_amdgcn_s_memrealtime();
#define XV_CLK_END(buf)                                                                   \
  {                                                                                       \
    const unsigned long long clk_m1 = __builtin_amdgcn_s_memtime();                       \
    const unsigned long long clk_r1 = __builtin_amdgcn_s_memrealtime();                   \
    if (threadIdx.x == 0 && blockIdx.x < XV_CLK_SLOTS) {                                  \
      buf[blockIdx.x * 4 + 0] = clk_m0, buf[blockIdx.x * 4 + 1] = clk_r0;                 \
      buf[blockIdx.x * 4 + 2] = clk_m1, buf[blockIdx.x * 4 + 3] = clk_r1;                 \
    }                                                                                     \
  }
#else
#define XV_CLK_BEGIN()
#define XV_CLK_END(buf)
#endif
