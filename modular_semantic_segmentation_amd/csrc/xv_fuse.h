// The staging of the fusion tables into LDS, the Dirichlet renormalise-and-log and the first-maximum decision of one pixel,
// written ONCE for the fusion kernels (fusion.hip, on materialised maps) and the fused heads (heads.hip, multi_count.hip, on
// registers): equal inputs give equal bits by construction, not by keeping copies alike.  That holds because contraction is
// by the SOURCE only (a * b + c inside one expression, never across statements; the pragma below, for the rest of the
// including file too).  Under -ffp-contract=fast the optimizer fuses a product into a later sum wherever the two meet: once,
// specialising the fused head on the class count removed a select between `p = e * rsum` and `sum += p`, it became an fma
// there and not in the kernel that reads p back from memory, and one pixel in a million flipped.
// NOT here, because the register allocation of these kernels got worse through force-inlined functions (the same statements
// reach the scheduler in another order): the Dirichlet fma chains with - lognorm (all classes at once: fused_head_kernel<20,
// 1, false> 81 -> 117 registers, fused_head_multi_kernel<12, 1, false> spilled 32 B; four classes at a time:
// fused_head_grid_score_kernel<12> 84 -> 97, five waves per SIMD -> four), fused_head_kernel's Dirichlet argmax (the same
// 81 -> 117), bayes_fuse2_kernel's decision table (42 -> 43).  Because they measured slower than the parent by more than its run-to-run
// gap: the Bayes path of fused_head_multi_kernel (2 %), fuse_renorm_log in its Dirichlet path (four experts 1.7 %), and every
// shared piece in fused_head_multi_count_kernel (0.7 to 1.8 %).  The tests that compare the routes hold those copies.
#pragma once

#include "xv_common.h"

#pragma clang fp contract(on)

typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- staging (every thread of a 256-thread workgroup calls them; the caller synchronises) ----------------------------------
// rows [nrows][C] -> [nrows][CM], zero padded: the Bayes log-likelihoods [E][C], the untransposed Dirichlet parameters
template <int CM>
__device__ static __forceinline__ void fuse_stage_rows(float* tab, const float* tab_g, int nrows, int C) {
  for (int i = threadIdx.x; i < nrows * CM; i += 256) {
    const int k = i % CM, row = i / CM;
    tab[i] = k < C ? tab_g[row * C + k] : 0.f;
  }
}

// one Dirichlet parameter set, TRANSPOSED: tab[(e CM + k) CM + c] = alpha_e[c][k] - 1, so that the dot products of a pixel
// advance together, two classes per v_pk_fma_f32; lognorm [E][CM]
template <int CM>
__device__ static __forceinline__ void fuse_stage_dirichlet(float* tab, float* ln, const float* tab_g,
                                                            const float* lognorm_g, int E, int C) {
  for (int i = threadIdx.x; i < E * CM * CM; i += 256) {
    const int c = i % CM, k = (i / CM) % CM, e = i / (CM * CM);
    tab[i] = (c < C && k < C) ? tab_g[(e * C + c) * C + k] : 0.f;
  }
  fuse_stage_rows<CM>(ln, lognorm_g, E, C);
}

// G Dirichlet parameter sets (grid points), each the transposed table [E][CM k][CM c], lognorm [E][CM], logprior [CM]
template <int CM>
__device__ static __forceinline__ void fuse_stage_dirichlet_points(float* dst, const float* tab_g,
                                                                   const float* lognorm_g,
                                                                   const float* logprior_g, int E, int G, int C) {
  const int PT = E * CM * CM + E * CM + CM;  // floats per point
  for (int i = threadIdx.x; i < G * PT; i += 256) {
    const int g = i / PT, r = i - g * PT;
    float v;
    if (r < E * CM * CM) {
      const int c = r % CM, k = (r / CM) % CM, e = r / (CM * CM);
      v = (c < C && k < C) ? tab_g[((g * E + e) * C + c) * C + k] : 0.f;
    } else if (r < E * CM * CM + E * CM) {
      const int q = r - E * CM * CM, k = q % CM, e = q / CM;
      v = k < C ? lognorm_g[(g * E + e) * C + k] : 0.f;
    } else {
      const int k = r - E * CM * CM - E * CM;
      v = k < C ? logprior_g[g * C + k] : 0.f;
    }
    dst[i] = v;
  }
}

// ---- the decision: first maximum over k < C of total[k] + lp[k] (Bayes, Dirichlet) or total[k] / fe (mean, an IEEE division)
template <int CM>
__device__ static __forceinline__ int fuse_argmax_prior(const float (&total)[CM], const float* lp, int C) {
  float best = 0.f;
  int bi = 0;
#pragma unroll
  for (int k = 0; k < CM; ++k) {
    const float v = total[k] + lp[k];
    if (k < C && (k == 0 || v > best)) {
      best = v;
      bi = k;
    }
  }
  return bi;
}

template <int CM>
__device__ static __forceinline__ int fuse_argmax_mean(const float (&total)[CM], float fe, int C) {
  float best = 0.f;
  int bi = 0;
#pragma unroll
  for (int k = 0; k < CM; ++k) {
    const float v = total[k] / fe;
    if (k < C && (k == 0 || v > best)) {
      best = v;
      bi = k;
    }
  }
  return bi;
}

// ---- Dirichlet: one expert's probabilities -> renormalised, log(1e-20 + p); classes past C become 0.  The product and the sum
// are ONE expression (an fma by the source), the sum before it a chain of separate adds: the statements the bit flip above came
// from.  MASK: x may hold anything past C (a row loader that pads with zeros needs no mask).
template <int CM, bool MASK>
__device__ static __forceinline__ void fuse_renorm_log(float (&x)[CM], int C) {
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < CM; ++k) {
    if (MASK) x[k] = k < C ? x[k] : 0.f;
    sum += x[k];
  }
  const float rs = xv_fast_rcp(sum);
#pragma unroll
  for (int k = 0; k < CM; ++k) x[k] = k < C ? xv_fast_log(1e-20f + x[k] * rs) : 0.f;
}
