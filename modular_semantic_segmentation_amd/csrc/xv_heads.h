// The per-pixel pieces of the inference heads (heads.hip) that other files count with (grouped_score.hip): the bilinear x8
// class scores of one output pixel from the low-resolution score map, their maximum, label and softmax, and the wave-aggregated
// LDS counter.  Every kernel that calls them executes the same arithmetic in the same order, so their labels are bit-identical.
#pragma once

#include "xv_common.h"
#include "xv_fuse.h"  // the fusion of a pixel; why equal inputs give equal bits is explained there

// Floating-point contraction by the SOURCE only (a * b + c inside one expression), never across statements, here and in the
// rest of a file that includes this one: see xv_fuse.h.
#pragma clang fp contract(on)

// Kernel 2: one thread per output pixel: 4-tap bilinear interpolation of the CM low-resolution class
// scores, + bias, softmax, argmax.  The per-pixel pieces are device functions shared with the fused two-expert head
// (fused_head_kernel), so both paths execute the same arithmetic in the same order: their labels are bit-identical.
// the four low-resolution score vectors around output pixel (oy, ox) (shared by the 4 output pixels ox = 4m .. 4m + 3:
// bilinear_taps<8> changes its source column at ox = 4 mod 8 only)
template <int CM>
__device__ static __forceinline__ void head_load_taps(const float* __restrict__ S, int n, int iy1, int ix1, int Hi, int Wi,
                                               f32x4 (&a)[CM / 4], f32x4 (&b)[CM / 4], f32x4 (&c)[CM / 4], f32x4 (&d)[CM / 4]) {
  // padded coords: logical source (iy1-1, ix1-1) is padded (iy1, ix1)
  const float* p00 = S + (((int64_t)n * (Hi + 2) + iy1) * (Wi + 2) + ix1) * CM;
  const int64_t rowp = (int64_t)(Wi + 2) * CM;
#pragma unroll
  for (int k4 = 0; k4 < CM / 4; ++k4) {
    a[k4] = *reinterpret_cast<const f32x4*>(p00 + 4 * k4);
    b[k4] = *reinterpret_cast<const f32x4*>(p00 + CM + 4 * k4);
    c[k4] = *reinterpret_cast<const f32x4*>(p00 + rowp + 4 * k4);
    d[k4] = *reinterpret_cast<const f32x4*>(p00 + rowp + CM + 4 * k4);
  }
}

// one class quad of the logits from its four taps: per class an explicit fmaf chain -- the ONE place it is written, so the
// unfused head, the fused heads and the quad-at-a-time walker below give identical bits by construction
template <int CM>
__device__ static __forceinline__ void head_eval_quad(const f32x4& a, const f32x4& b, const f32x4& c, const f32x4& d, float w00,
                                                      float w01, float w10, float w11, int k4, float (&sc)[CM]) {
  sc[4 * k4] = fmaf(d.x, w11, fmaf(c.x, w10, fmaf(b.x, w01, a.x * w00)));
  sc[4 * k4 + 1] = fmaf(d.y, w11, fmaf(c.y, w10, fmaf(b.y, w01, a.y * w00)));
  sc[4 * k4 + 2] = fmaf(d.z, w11, fmaf(c.z, w10, fmaf(b.z, w01, a.z * w00)));
  sc[4 * k4 + 3] = fmaf(d.w, w11, fmaf(c.w, w10, fmaf(b.w, w01, a.w * w00)));
}

// logits of one output pixel from its taps (head_eval_quad per class quad), then the bias
template <int CM>
__device__ static __forceinline__ void head_eval_taps(const f32x4 (&a)[CM / 4], const f32x4 (&b)[CM / 4], const f32x4 (&c)[CM / 4],
                                               const f32x4 (&d)[CM / 4], float wy1, float wy0, float wx1, float wx0,
                                               const float* __restrict__ bs_g, int C, float (&sc)[CM]) {
  const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
#pragma unroll
  for (int k4 = 0; k4 < CM / 4; ++k4) head_eval_quad<CM>(a[k4], b[k4], c[k4], d[k4], w00, w01, w10, w11, k4, sc);
#pragma unroll
  for (int k = 0; k < CM; ++k) sc[k] += bs_g[k < C ? k : C - 1];
}

// head_load_taps + head_eval_taps a class quad at a time (16 registers of taps instead of 4 CM; multi_count.hip's wide
// four-expert forms).  A quad's loads wait for the quad before (their address depends on its last score: an empty asm, no
// instruction), otherwise the scheduler asks for all of them at once and nothing is saved.
template <int CM>
__device__ static __forceinline__ void head_logits_quads(const float* __restrict__ S, const float* __restrict__ bs_g, int n, int iy1,
                                                         int ix1, int Hi, int Wi, float wy1, float wy0, float wx1, float wx0, int C,
                                                         float (&sc)[CM]) {
  const float* p00 = S + (((int64_t)n * (Hi + 2) + iy1) * (Wi + 2) + ix1) * CM;
  const int64_t rowp = (int64_t)(Wi + 2) * CM;
  const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
#pragma unroll
  for (int k4 = 0; k4 < CM / 4; ++k4) {
    int off = 0;
    if (k4 > 0) asm volatile("" : "+v"(off) : "v"(sc[k4 > 0 ? 4 * k4 - 1 : 0]));
    const float* p = p00 + off;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * k4);
    const f32x4 b = *reinterpret_cast<const f32x4*>(p + CM + 4 * k4);
    const f32x4 c = *reinterpret_cast<const f32x4*>(p + rowp + 4 * k4);
    const f32x4 d = *reinterpret_cast<const f32x4*>(p + rowp + CM + 4 * k4);
    head_eval_quad<CM>(a, b, c, d, w00, w01, w10, w11, k4, sc);
  }
#pragma unroll
  for (int k = 0; k < CM; ++k) sc[k] += bs_g[k < C ? k : C - 1];
}

template <int CM>
__device__ static __forceinline__ void head_logits(const float* __restrict__ S, const float* __restrict__ bs_g, int n, int oy, int ox,
                                            int Hi, int Wi, int C, float (&sc)[CM]) {
  int iy1, ix1;
  float wy1, wy0, wx1, wx0;
  bilinear_taps<8>(oy, iy1, wy1, wy0);
  bilinear_taps<8>(ox, ix1, wx1, wx0);
  f32x4 a[CM / 4], b[CM / 4], c[CM / 4], d[CM / 4];
  head_load_taps<CM>(S, n, iy1, ix1, Hi, Wi, a, b, c, d);
  head_eval_taps<CM>(a, b, c, d, wy1, wy0, wx1, wx0, bs_g, C, sc);
}

template <int CM>
__device__ static __forceinline__ float head_max(const float (&sc)[CM], int C) {
  float m = sc[0];
#pragma unroll
  for (int k = 1; k < CM; ++k)
    if (k < C) m = fmaxf(m, sc[k]);
  return m;
}

// labels only (the experts of a Bayes fusion): argmax(softmax(x)) is argmax(x) unless the runner-up is so close that
// the two probabilities round to the same float (|difference| < ~1e-7); only then does the reference's tie rule
// (lowest index among equal PROBABILITIES) need the probabilities themselves.  Returns -1 in that case.
template <int CM>
__device__ static __forceinline__ int head_label_fast(const float (&sc)[CM], float m, int C) {
  // exactly one k with (m - sc[k]) <= 1e-5 (the maximum itself)  <=>  the SECOND largest value, duplicates counted, is more
  // than 1e-5 below m (the subtraction is monotone in sc[k]): s2 = med3(s1, s2, x) under the running maximum s1.  Counting the
  // near classes cost a subtraction, a compare and an add per class: 2 242 -> 1 822 vector instructions in the fused Bayes head.
  float s1 = sc[0], s2 = -__builtin_inff();
  int bi = 0;
#pragma unroll
  for (int k = 1; k < CM; ++k)
    if (k < C) {
      s2 = __builtin_amdgcn_fmed3f(s1, s2, sc[k]);
      s1 = fmaxf(s1, sc[k]);
    }
#pragma unroll
  for (int k = CM - 1; k >= 0; --k)
    if (k < C && sc[k] == m) bi = k;
  return (m - s2) <= 1e-5f ? -1 : bi;
}

// sc <- softmax(sc) (tf.nn.softmax: exp(x - max) / sum); returns the label, lowest index on ties
template <int CM>
__device__ static __forceinline__ int head_softmax(float (&sc)[CM], float m, int C) {
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < CM; ++k) {
    sc[k] = k < C ? xv_fast_exp(sc[k] - m) : 0.f;
    sum += sc[k];
  }
  const float rsum = xv_fast_rcp(sum);
  float best = -1.f;
  int bi = 0;
#pragma unroll
  for (int k = 0; k < CM; ++k) {
    sc[k] = sc[k] * rsum;
    if (k < C && sc[k] > best) {
      best = sc[k];
      bi = k;
    }
  }
  return bi;
}

// One wave's keys -> LDS counters.  Neighbouring pixels agree on (label, prediction), so up to 64 lanes of a wave would meet on
// one counter; equal keys are aggregated first: the lowest pending lane's key is broadcast, the lanes holding it are counted by
// a ballot, that lane alone adds the count, and the loop runs once per DISTINCT key of the wave (one to three on segmentation
// maps, at most 64).  Exact whatever the keys are, and it needs no table copies, which is what leaves the LDS to the grid
// points.  key < 0: nothing to count.  Every lane of the wave calls it, in converged control flow.
__device__ static __forceinline__ void xv_wave_count(uint32_t* cells, int key) {
  unsigned long long todo = __ballot(key >= 0);
  const int lane = (int)__lane_id();
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const int k0 = __builtin_amdgcn_readlane(key, leader);
    const unsigned long long same = __ballot(key == k0);
    if (lane == leader) atomicAdd(&cells[k0], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

// output pixels per thread of the joint-histogram heads: four up to 12 classes, two above (fused_head_joint_hist_kernel)
constexpr int xv_joint_hist_pixels(int cm) { return cm <= 12 ? 4 : 2; }

// Score and bias pointers of the two to four experts of fused_head_multi_kernel (heads.hip) and its counting form
// (multi_count.hip), as kernel arguments: no pointer table in device memory.
constexpr int XV_MULTI_MAXE = 4;
struct HeadPtrs {
  const float* s[XV_MULTI_MAXE];
  const float* b[XV_MULTI_MAXE];
};

// (selects on a wave-uniform index: a kernel argument array indexed at run time must not become a private copy)
__device__ static __forceinline__ const float* head_ptr(const float* const (&p)[XV_MULTI_MAXE], int e) {
  return e == 0 ? p[0] : (e == 1 ? p[1] : (e == 2 ? p[2] : p[3]));
}
