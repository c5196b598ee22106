// Inference heads of the FCN and the fusion models for gfx950: the low-resolution score conv, the decoder heads (bilinear x8 +
// relu + 1x1 score + softmax + argmax), the fused two-expert, variance and uncertainty heads, and the dense softmax + argmax.
#include <stdlib.h>

#include "xv_common.h"
#include "xv_heads.h"
#include "xv_multi.h"  // the host side of the multi-expert head: argument checks, the grid bound

// Floating-point contraction by the SOURCE only (a * b + c inside one expression), never across statements: the fused heads
// and the unfused path (decoder head -> probability maps -> fusion kernel) must produce the same bits; see xv_fuse.h.
#pragma clang fp contract(on)

namespace {

// ---- decoder head: bilinear x8 + relu + 1x1 score + softmax + argmax ----------------------------
// simple_fcn.py:129-133 + basic_fusion_model.py:21-22.
//
// `fused` = relu(score_conv4) + relu(bilinear_x2(..)) is non-negative by construction and the
// bilinear weights are positive, so relu(bilinear_x8(fused)) == bilinear_x8(fused): the x8 deconv and
// the 1x1 `score` conv are both linear and commute.  The head therefore runs the 1x1 conv at 1/8
// resolution (U -> C channels on h*w pixels instead of 64*h*w) and interpolates C class scores instead
// of U features: 16x fewer FMAs per output pixel, same value up to fp32 summation order.  The bias is
// added after the interpolation (at the image border the zero-padded bilinear weights do not sum to 1).
//
// Kernel 1: S[n][i][j][k] = sum_u fused[n,i,j,u] * Ws[u][k] into a zero-bordered fp32 [N][h+2][w+2][CP]
// workspace (CP = C rounded up to 4).  Score weights sit zero-padded in LDS and are read with wave-uniform
// (broadcast) addresses.
template <int CM>
__global__ __launch_bounds__(128) void score_lowres_kernel(const __bf16* __restrict__ f, const float* __restrict__ ws_g,
                                                          int N, int Hi, int Wi, int U, int C, float* __restrict__ S) {
  extern __shared__ __attribute__((aligned(16))) float wsm[];  // [U][CM], zero padded
  for (int i = threadIdx.x; i < U * CM; i += 128) {
    const int u = i / CM, k = i - u * CM;
    wsm[i] = k < C ? ws_g[u * C + k] : 0.f;
  }
  __syncthreads();
  const int64_t total = (int64_t)N * (Hi + 2) * (Wi + 2);
  const int64_t pp = (int64_t)blockIdx.x * 128 + threadIdx.x;  // padded pixel index (same geometry as `fused`)
  if (pp >= total) return;
  const int x = (int)(pp % (Wi + 2));
  const int y = (int)((pp / (Wi + 2)) % (Hi + 2));
  float sc[CM];
#pragma unroll
  for (int k = 0; k < CM; ++k) sc[k] = 0.f;
  const bool interior = x >= 1 && x <= Wi && y >= 1 && y <= Hi;
  if (interior) {
    const __bf16* src = f + pp * U;
    for (int u0 = 0; u0 < U; u0 += 8) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(src + u0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float fv = bf16_bits_to_f32((v[i >> 1] >> ((i & 1) * 16)) & 0xffffu);
        const float* wrow = wsm + (u0 + i) * CM;  // wave-uniform address: LDS broadcast reads
#pragma unroll
        for (int k4 = 0; k4 < CM; k4 += 4) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wrow + k4);
          sc[k4] = fmaf(fv, wv.x, sc[k4]);
          sc[k4 + 1] = fmaf(fv, wv.y, sc[k4 + 1]);
          sc[k4 + 2] = fmaf(fv, wv.z, sc[k4 + 2]);
          sc[k4 + 3] = fmaf(fv, wv.w, sc[k4 + 3]);
        }
      }
    }
  }
  float* dst = S + pp * CM;
#pragma unroll
  for (int k4 = 0; k4 < CM; k4 += 4) *reinterpret_cast<f32x4*>(dst + k4) = f32x4{sc[k4], sc[k4 + 1], sc[k4 + 2], sc[k4 + 3]};
}

// Kernel 2: one thread per output pixel (decoder_head_kernel below); its per-pixel pieces -- head_load_taps, head_eval_taps,
// head_logits, head_max, head_label_fast, head_softmax -- live in xv_heads.h.

template <int CM>
__global__ __launch_bounds__(256) void decoder_head_kernel(const float* __restrict__ S, const float* __restrict__ bs_g,
                                                          int N, int Hi, int Wi, int C, float* __restrict__ score,
                                                          float* __restrict__ prob, int64_t* __restrict__ label) {
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t npix = (int64_t)N * Ho * Wo;
  const int64_t opix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (opix >= npix) return;
  const int ox = (int)(opix % Wo);
  const int oy = (int)((opix / Wo) % Ho);
  const int n = (int)(opix / ((int64_t)Wo * Ho));
  float sc[CM];
  head_logits<CM>(S, bs_g, n, oy, ox, Hi, Wi, C, sc);
  if (score) {
#pragma unroll
    for (int k = 0; k < CM; ++k)
      if (k < C) score[opix * C + k] = sc[k];
  }
  if (prob || label) {
    const float m = head_max<CM>(sc, C);
    if (!prob) {
      const int fast = head_label_fast<CM>(sc, m, C);
      if (fast >= 0) {
        label[opix] = fast;
        return;
      }
    }
    const int bi = head_softmax<CM>(sc, m, C);
    if (prob) {
#pragma unroll
      for (int k = 0; k < CM; ++k)
        if (k < C) prob[opix * C + k] = sc[k];
    }
    if (label) label[opix] = bi;
  }
}

// decoder_head_kernel for the label alone, FOUR consecutive output pixels ox = 4m .. 4m + 3 per thread: they share their four
// low-resolution source vectors (bilinear_taps<8> changes its source column at ox = 4 mod 8 only) and leave as two 16-byte
// stores -- the same device functions per pixel, so the same labels.  16 images of 768x384, score_lowres + head: 44 -> 33 us
// (one pixel per thread issued 12 16-byte loads for every 8-byte result).
template <int CM>
__global__ __launch_bounds__(256) void decoder_head_label4_kernel(const float* __restrict__ S, const float* __restrict__ bs_g,
                                                                 int N, int Hi, int Wi, int C, int64_t* __restrict__ label) {
  const int Ho = Hi * 8, Wo = Wi * 8, Wq = Wo / 4;
  const int64_t nquads = (int64_t)N * Ho * Wq;
  const int64_t quad = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (quad >= nquads) return;
  const int ox0 = (int)(quad % Wq) * 4;
  const int oy = (int)((quad / Wq) % Ho);
  const int n = (int)(quad / ((int64_t)Wq * Ho));
  int iy1, ix1;
  float wy1, wy0;
  bilinear_taps<8>(oy, iy1, wy1, wy0);
  {
    float u1, u0;
    bilinear_taps<8>(ox0, ix1, u1, u0);
  }
  f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
  head_load_taps<CM>(S, n, iy1, ix1, Hi, Wi, ta, tb, tc, td);
  int64_t out[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int ixp;
    float wx1, wx0;
    bilinear_taps<8>(ox0 + p, ixp, wx1, wx0);
    float sc[CM];
    head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, bs_g, C, sc);
    const float m = head_max<CM>(sc, C);
    int l = head_label_fast<CM>(sc, m, C);
    if (l < 0) l = head_softmax<CM>(sc, m, C);
    out[p] = l;
  }
  typedef __attribute__((ext_vector_type(2))) long long i64x2;
  int64_t* dst = label + quad * 4;
  *reinterpret_cast<i64x2*>(dst) = i64x2{out[0], out[1]};
  *reinterpret_cast<i64x2*>(dst + 2) = i64x2{out[2], out[3]};
}

// ---- fused two-expert head: both experts' low-resolution class scores -> per-pixel logits -> softmax / argmax of
// each expert -> Bayes (bayes_mix.py:33-58) or Dirichlet (dirichlet_mix.py:14-36,96-136) fusion -> ONE fused label.
// Replaces, for the default prediction of a two-expert fusion model, two decoder_head launches + the fusion kernel and
// every per-pixel intermediate between them (Bayes: two int64 label maps written and read back; Dirichlet: two fp32
// probability maps, 2 x 4C B per pixel each way).  The fusion arithmetic is the one of fusion.hip's kernels, term for
// term (staging and fuse_renorm_log shared through xv_fuse.h; the fma chains written out here, see there), on the values
// the unfused path would have stored.  Tables in LDS: tab [2][C][CM], lognorm [2][CM] (Dirichlet), logprior [CM], dec [C][C]
// (Bayes: the decision per label pair, built by the workgroup).
// FULL: the class count IS CM (the 12 classes of the headline model): every `k < C` folds away -- 165 of the Dirichlet
// form's ~800 vector instructions per pixel were compare-selects on the run-time class count.
template <int CM, int DIRICHLET, bool FULL = false, int P = (DIRICHLET ? 1 : 4)>
__global__ __launch_bounds__(256) void fused_head_kernel(const float* __restrict__ Sa, const float* __restrict__ Sb,
                                                        const float* __restrict__ ba, const float* __restrict__ bb, int N,
                                                        int Hi, int Wi, int C_, const float* __restrict__ tab_g,
                                                        const float* __restrict__ lognorm_g,
                                                        const float* __restrict__ logprior_g, int64_t* __restrict__ fused) {
  const int C = FULL ? CM : C_;
  extern __shared__ __attribute__((aligned(16))) float tab[];
  float* ln = tab + (DIRICHLET ? 2 * CM * CM : 2 * C * CM);
  float* lp = ln + 2 * CM;
  if constexpr (DIRICHLET) {
    fuse_stage_dirichlet<CM>(tab, ln, tab_g, lognorm_g, 2, C);
  } else {
    fuse_stage_rows<CM>(tab, tab_g, 2 * C, C);
    for (int i = threadIdx.x; i < 2 * CM; i += 256) ln[i] = 0.f;
  }
  if (threadIdx.x < CM) lp[threadIdx.x] = threadIdx.x < C ? logprior_g[threadIdx.x] : 0.f;
  __syncthreads();
  // Bayes: the fused label is a function of the two experts' labels alone -- dec[a][b] = argmax_k (tab_0[a][k] + tab_1[b][k] +
  // logprior[k]), built here by the workgroup with the sums in the order of bayes_fuse_kernel (fusion.hip; as bayes_fuse2_kernel
  // does for the unfused path): a pixel is then ONE 4-byte LDS lookup instead of six lane-varying 16-byte row reads, 36 adds
  // and a 12-way argmax chain, and the thread keeps two labels per pixel instead of CM sums.
  int* dec = reinterpret_cast<int*>(lp + CM);  // [C][C]
  if constexpr (!DIRICHLET) {
    for (int i = threadIdx.x; i < C * C; i += 256) {
      const float* ra = tab + (i / C) * CM;
      const float* rb = tab + (C + i % C) * CM;
      float best = 0.f;
      int bi = 0;
      for (int k = 0; k < C; ++k) {
        float sc = ra[k];
        sc = sc + rb[k];
        const float v = sc + lp[k];
        if (k == 0 || v > best) {
          best = v;
          bi = k;
        }
      }
      dec[i] = bi;
    }
    __syncthreads();
  }
  // Bayes: one thread = P = FOUR consecutive output pixels ox = 4m .. 4m + 3: they share their four low-resolution source
  // vectors (24 16-byte loads per expert pair instead of 96) and leave as two 16-byte stores: 71.8 -> 54.6 us for 37.7 MB
  // at 16 images of 768x384 (profiles/r3_elementwise.json: not HBM-bound, 0.10 of the HBM rate: the per-pixel argmax
  // chains and the lane-varying table reads in LDS remain).  Dirichlet (24 logs + 288 FMAs per pixel, 48 more live
  // registers per extra pixel) keeps one pixel per thread in this scalar form: four measured 14 % slower.  (C == CM runs
  // fused_dirichlet_head_pk_kernel below.)
  const int Ho = Hi * 8, Wo = Wi * 8, Wq = Wo / P;
  const int64_t nquads = (int64_t)N * Ho * Wq;
  const int64_t quad = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (quad >= nquads) return;
  const int ox0 = (int)(quad % Wq) * P;
  const int oy = (int)((quad / Wq) % Ho);
  const int n = (int)(quad / ((int64_t)Wq * Ho));
  int iy1, ix1;
  float wy1, wy0;
  bilinear_taps<8>(oy, iy1, wy1, wy0);
  float total[P][CM];
  int lab[2][P];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
    {
      float u1, u0;
      bilinear_taps<8>(ox0, ix1, u1, u0);
    }
    head_load_taps<CM>(e == 0 ? Sa : Sb, n, iy1, ix1, Hi, Wi, ta, tb, tc, td);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      int ixp;
      float wx1, wx0;
      bilinear_taps<8>(ox0 + p, ixp, wx1, wx0);
      float sc[CM];
      head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, e == 0 ? ba : bb, C, sc);
      const float m = head_max<CM>(sc, C);
      if (!DIRICHLET) {
        int l = head_label_fast<CM>(sc, m, C);
        if (l < 0) l = head_softmax<CM>(sc, m, C);
        lab[e][p] = l;
      } else {
        head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
        fuse_renorm_log<CM, true>(sc, C);
        // The C dot products sum_k (alpha[c][k] - 1) log p[k], each the fmaf chain over k of dirichlet_fuse_kernel (bit for
        // bit), advanced TWO CLASSES PER INSTRUCTION: v_pk_fma_f32 on the transposed table halves the 2 C^2 = 288 FMAs that
        // made this kernel VALU-bound (padded classes / terms are exact zeros: fma(0, 0, d) = d).
        f32x2 dot2[CM / 2];
#pragma unroll
        for (int cp = 0; cp < CM / 2; ++cp) dot2[cp] = f32x2{0.f, 0.f};
#pragma unroll
        for (int k = 0; k < CM; ++k) {
          const f32x2* rowk = reinterpret_cast<const f32x2*>(tab + (e * CM + k) * CM);
          const f32x2 lk = f32x2{sc[k], sc[k]};
#pragma unroll
          for (int cp = 0; cp < CM / 2; ++cp) dot2[cp] = __builtin_elementwise_fma(rowk[cp], lk, dot2[cp]);
        }
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          const float L = dot2[c >> 1][c & 1] - ln[e * CM + c];
          total[p][c] = c < C ? (e == 0 ? L : total[p][c] + L) : 0.f;
        }
      }
    }
  }
  int64_t out[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if constexpr (!DIRICHLET) {
      out[p] = dec[lab[0][p] * C + lab[1][p]];
    } else {
      // (fuse_argmax_prior of xv_fuse.h, written out: through it the 20-class forms take 78 / 117 registers for 74 / 81)
      float best = 0.f;
      int bi = 0;
#pragma unroll
      for (int k = 0; k < CM; ++k) {
        const float v = total[p][k] + lp[k];
        if (k < C && (k == 0 || v > best)) {
          best = v;
          bi = k;
        }
      }
      out[p] = bi;
    }
  }
  int64_t* dst = fused + (quad * P);
  if constexpr (P == 4) {
    typedef __attribute__((ext_vector_type(2))) long long i64x2;
    *reinterpret_cast<i64x2*>(dst) = i64x2{out[0], out[1]};
    *reinterpret_cast<i64x2*>(dst + 2) = i64x2{out[2], out[3]};
  } else {
#pragma unroll
    for (int p = 0; p < P; ++p) dst[p] = out[p];
  }
}

// ---- variance head of the MC-dropout fusion model (variance_mix.py:7-15,33-83): both experts' low-resolution class scores of
// T + 1 passes each (slot-major: images 0 .. N-1 are the plain pass, t N .. t N + N-1 dropout sample t; xv_score_lowres of the
// (T+1) N-image maps) -> per output pixel and expert: the probabilities p_t of every sample (head_logits / head_max /
// head_softmax: the bits of decoder_head_kernel's `prob`), their population variance over the T samples per class
// (tf.nn.moments over the sample axis) averaged over the classes, and the probabilities of the plain pass -> the
// certainty-weighted fusion (xv_variance_fuse_add / _finish, shared with xv_variance_fuse) -> the fused label.  The moments
// take two passes over the samples, each RECOMPUTING p_t from the taps (nothing of size T C is held): the mean of the
// deviations d_t = p_t - p_1 from the first sample, then the mean of (d_t - mean)^2 -- the variance of p itself; shifting by a
// sample keeps identical samples at a variance of exactly 0 (the mean of T equal fp32 values, summed and scaled, need not be
// that value).  Optional outputs: fused score [N][8Hi][8Wi][C], plain probabilities [2][N][8Hi][8Wi][C], variance
// [2][N][8Hi][8Wi].  One output pixel per thread.
template <int CM>
__device__ __forceinline__ void head_prob(const float* __restrict__ S, const float* __restrict__ bs_g, int n, int oy, int ox,
                                          int Hi, int Wi, int C, float (&sc)[CM]) {
  head_logits<CM>(S, bs_g, n, oy, ox, Hi, Wi, C, sc);
  const float m = head_max<CM>(sc, C);
  head_softmax<CM>(sc, m, C);
}

template <int CM>
__global__ __launch_bounds__(256) void variance_head_kernel(const float* __restrict__ Sa, const float* __restrict__ Sb,
                                                           const float* __restrict__ ba, const float* __restrict__ bb, int N,
                                                           int Hi, int Wi, int C, int T, int64_t* __restrict__ label,
                                                           float* __restrict__ score, float* __restrict__ prob,
                                                           float* __restrict__ var_out) {
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t npix = (int64_t)N * Ho * Wo;
  const int64_t opix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (opix >= npix) return;
  const int ox = (int)(opix % Wo);
  const int oy = (int)((opix / Wo) % Ho);
  const int n = (int)(opix / ((int64_t)Wo * Ho));
  const float invT = 1.f / (float)T;
  const float invTC = 1.f / (float)(T * C);
  float var[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float* S = e == 0 ? Sa : Sb;
    const float* bs = e == 0 ? ba : bb;
    float p1[CM], mean[CM], sc[CM];
    head_prob<CM>(S, bs, N + n, oy, ox, Hi, Wi, C, p1);
#pragma unroll
    for (int k = 0; k < CM; ++k) mean[k] = 0.f;
    for (int t = 2; t <= T; ++t) {
      head_prob<CM>(S, bs, t * N + n, oy, ox, Hi, Wi, C, sc);
#pragma unroll
      for (int k = 0; k < CM; ++k) mean[k] += sc[k] - p1[k];
    }
    float sq[CM];
#pragma unroll
    for (int k = 0; k < CM; ++k) {
      mean[k] = mean[k] * invT;
      sq[k] = mean[k] * mean[k];  // sample 1: d_1 = 0
    }
    for (int t = 2; t <= T; ++t) {
      head_prob<CM>(S, bs, t * N + n, oy, ox, Hi, Wi, C, sc);
#pragma unroll
      for (int k = 0; k < CM; ++k) {
        const float d = (sc[k] - p1[k]) - mean[k];
        sq[k] = __builtin_fmaf(d, d, sq[k]);
      }
    }
    float vs = 0.f;
#pragma unroll
    for (int k = 0; k < CM; ++k)
      if (k < C) vs += sq[k];
    var[e] = vs * invTC;
  }
  float acc[CM], csum;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    float sc[CM];
    head_prob<CM>(e == 0 ? Sa : Sb, e == 0 ? ba : bb, n, oy, ox, Hi, Wi, C, sc);
    if (prob) {
      float* dst = prob + ((int64_t)e * npix + opix) * C;
#pragma unroll
      for (int k = 0; k < CM; ++k)
        if (k < C) dst[k] = sc[k];
    }
    if (var_out) var_out[(int64_t)e * npix + opix] = var[e];
    xv_variance_fuse_add<CM>(acc, csum, sc, var[e], e == 0);
  }
  const int l = xv_variance_fuse_finish<CM>(acc, csum, C);
  label[opix] = l;
  if (score) {
#pragma unroll
    for (int k = 0; k < CM; ++k)
      if (k < C) score[opix * C + k] = acc[k];
  }
}

// ---- uncertainty head of the MC-dropout Bayesian FCN (bayesian_fcn.py:48-57, custom_layers.py:251-256): ONE expert's
// low-resolution class scores of T dropout samples (sample-major: images t N .. t N + N-1 are sample t = 0 .. T-1, no plain
// slot; xv_score_lowres of the T N-image map) -> per output pixel the probabilities p_t of every sample (head_prob: the bits of
// decoder_head_kernel's `prob`), then
//   mean = (1/T) sum_t p_t, label = argmax mean (lowest index on ties), entropy = H(mean) / ln C,
//   cond_entropy = (1/T) sum_t H(p_t) / ln C, variance = sum_c population variance of p_tc over t,
// through xv_mc_first / xv_mc_add / xv_mc_finish (xv_common.h; shared with xv_sampling_uncertainty, which therefore gives the
// same bits on materialised p_t).  Numerics, fixed there: samples in ascending t, classes in ascending c; ONE pass, every
// sample interpolated once, Welford's running mean and sum of squared deviations (identical samples: variance exactly 0, mean
// exactly p_1; variance clamped at 0); T = 1: variance 0 and entropy == cond_entropy bit for bit.  Nothing of size T C is
// held: the running mean, the squared deviations and the current sample -- one register row fewer than variance_head_kernel.
// The four float outputs are optional; a launch without `cond_entropy` takes no logarithm per sample, one without `variance`
// keeps no second moment.
template <int CM>
__global__ __launch_bounds__(256) void mc_uncertainty_head_kernel(const float* __restrict__ S, const float* __restrict__ bs,
                                                                 int N, int Hi, int Wi, int C, int T, float ln_c,
                                                                 int64_t* __restrict__ label, float* __restrict__ mean_out,
                                                                 float* __restrict__ ent_out, float* __restrict__ cond_out,
                                                                 float* __restrict__ var_out) {
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t npix = (int64_t)N * Ho * Wo;
  const int64_t opix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (opix >= npix) return;
  const int ox = (int)(opix % Wo);
  const int oy = (int)((opix / Wo) % Ho);
  const int n = (int)(opix / ((int64_t)Wo * Ho));
  const bool want_ce = cond_out != nullptr, want_var = var_out != nullptr;
  float mean[CM], m2[CM], sc[CM], ce;
  head_prob<CM>(S, bs, n, oy, ox, Hi, Wi, C, sc);
  xv_mc_first<CM>(mean, m2, ce, sc, C, want_ce);
  for (int t = 1; t < T; ++t) {
    head_prob<CM>(S, bs, t * N + n, oy, ox, Hi, Wi, C, sc);
    xv_mc_add<CM>(mean, m2, ce, sc, t + 1, C, want_ce, want_var);
  }
  float ent, cond, var;
  label[opix] = xv_mc_finish<CM>(mean, m2, ce, T, C, ln_c, ent_out != nullptr, ent, cond, var);
  if (mean_out) {
#pragma unroll
    for (int k = 0; k < CM; ++k)
      if (k < C) mean_out[opix * C + k] = mean[k];
  }
  if (ent_out) ent_out[opix] = ent;
  if (cond_out) cond_out[opix] = cond;
  if (var_out) var_out[opix] = var;
}

// ---- scoring form of the uncertainty head (uncertainty_model.py; experiments/uncertainty_eval.py:18-52,62-88): the per-pixel
// work of mc_uncertainty_head_kernel, statement for statement (head_logits / head_max / head_softmax per sample, then
// xv_mc_first / xv_mc_add / xv_mc_finish with every output wanted), with custom_layers.py:239-248's temperature: every
// interpolated logit times inv_temperature before the softmax (1.0f multiplies exactly: the bits of the head above; a power of
// two scales exactly: temperature 2 on S, bias is temperature 1 on S / 2, bias / 2).  The pixel's three values, its label and
// mean[label] go straight into the workgroup's replicated LDS tables (xv_common.h: nll / counts [C], hist [3][2][bins] in the
// order entropy, cond_entropy, variance; copy = lane & (rep - 1) fastest) -- NO map reaches HBM.  row = (argmax != label)
// over the pixels with 0 <= label < C, or the caller's fixed row over every pixel; NLL over the valid pixels either way.  A
// bounded grid (four 256-thread workgroups per CU, the four waves per SIMD of the register budget), pixels in a grid-stride
// loop, one global atomic per non-zero cell and workgroup.
template <int CM>
__device__ __forceinline__ void head_prob_scaled(const float* __restrict__ S, const float* __restrict__ bs_g, int n, int oy, int ox,
                                                 int Hi, int Wi, int C, float inv_t, float (&sc)[CM]) {
  head_logits<CM>(S, bs_g, n, oy, ox, Hi, Wi, C, sc);
#pragma unroll
  for (int k = 0; k < CM; ++k) sc[k] = sc[k] * inv_t;
  const float m = head_max<CM>(sc, C);
  head_softmax<CM>(sc, m, C);
}

template <int CM>
__global__ __launch_bounds__(256) void mc_uncertainty_score_kernel(const float* __restrict__ S, const float* __restrict__ bs, int N,
                                                                  int Hi, int Wi, int C, int T, float ln_c, float inv_t,
                                                                  const int32_t* __restrict__ labels, int M, int octaves,
                                                                  int fixed_row, unsigned long long* __restrict__ hist,
                                                                  double* __restrict__ nll, unsigned long long* __restrict__ counts,
                                                                  int XV_REP) {
  extern __shared__ __attribute__((aligned(16))) double unc_nll[];  // nll [C][XV_REP], cnt [C][XV_REP], hist [3][2][bins][XV_REP]
  const int ncls = labels ? C : 0, bins = octaves << M;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(unc_nll + ncls * XV_REP);
  uint32_t* hs = reinterpret_cast<uint32_t*>(unc_nll + 2 * ncls * XV_REP);
  xv_unc_tables_zero(unc_nll, ncls, hs, 6 * bins, XV_REP);
  __syncthreads();
  const int rep = threadIdx.x & (XV_REP - 1);
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t npix = (int64_t)N * Ho * Wo;
  for (int64_t opix = (int64_t)blockIdx.x * 256 + threadIdx.x; opix < npix; opix += (int64_t)gridDim.x * 256) {
    const int ox = (int)(opix % Wo);
    const int oy = (int)((opix / Wo) % Ho);
    const int n = (int)(opix / ((int64_t)Wo * Ho));
    float mean[CM], m2[CM], sc[CM], ce;
    head_prob_scaled<CM>(S, bs, n, oy, ox, Hi, Wi, C, inv_t, sc);
    xv_mc_first<CM>(mean, m2, ce, sc, C, true);
    for (int t = 1; t < T; ++t) {
      head_prob_scaled<CM>(S, bs, t * N + n, oy, ox, Hi, Wi, C, inv_t, sc);
      xv_mc_add<CM>(mean, m2, ce, sc, t + 1, C, true, true);
    }
    float ent, cond, var;
    const int bi = xv_mc_finish<CM>(mean, m2, ce, T, C, ln_c, true, ent, cond, var);
    const int l = labels ? labels[opix] : -1;
    const bool valid = l >= 0 && l < C;
    if (fixed_row >= 0 || valid) {
      const int row = fixed_row >= 0 ? fixed_row : (bi != l);
      atomicAdd(&hs[(row * bins + xv_unc_bin(ent, M, octaves)) * XV_REP + rep], 1u);
      atomicAdd(&hs[((2 + row) * bins + xv_unc_bin(cond, M, octaves)) * XV_REP + rep], 1u);
      atomicAdd(&hs[((4 + row) * bins + xv_unc_bin(var, M, octaves)) * XV_REP + rep], 1u);
    }
    if (valid) {
      float pl = mean[0];  // mean[l] by selects: statically indexed registers
#pragma unroll
      for (int k = 1; k < CM; ++k) pl = k == l ? mean[k] : pl;
      atomicAdd(&unc_nll[l * XV_REP + rep], xv_unc_nll_term(pl));
      atomicAdd(&cnt[l * XV_REP + rep], 1ull);
    }
  }
  __syncthreads();
  xv_unc_tables_flush(unc_nll, ncls, hs, 6 * bins, XV_REP, hist, nll, counts);
}

// ---- uncertainty-weighted Dirichlet fusion (uncertainty_dirichlet_mix.py:18-52,221-233): moments pass and fusion head ------
// Moments: both experts' low-resolution class scores of T + 1 passes (slot 0 plain, slots 1 .. T input-dropout samples; the
// contract of variance_head_kernel) -> per expert mvar [2][N][8Hi][8Wi], the population variance of every class's probability
// over the T samples averaged over the classes, and vmax [2], the largest per-class variance of the expert's whole tensor (the
// reference's reduce_max over pixels, classes AND images).  The per-pixel moments are variance_head_kernel's two sweeps about
// sample 1, statement for statement, so mvar carries the bits of that kernel's `variance`.  vmax is a grid-wide maximum that
// ends on two addresses: a bounded grid (at most 256 workgroups of 512 threads per expert: every CU at four waves per SIMD),
// pixels in a grid-stride loop, the running maximum in a register, one atomic per workgroup (xv_block_max_nonneg).  The entry
// point zeroes vmax.
template <int CM>
__device__ __forceinline__ float head_sample_moments(const float* __restrict__ S, const float* __restrict__ bs, int N, int n, int oy,
                                                     int ox, int Hi, int Wi, int C, int T, float invT, float invTC,
                                                     float& vmax_class) {
  float p1[CM], mean[CM], sc[CM];
  head_prob<CM>(S, bs, N + n, oy, ox, Hi, Wi, C, p1);
#pragma unroll
  for (int k = 0; k < CM; ++k) mean[k] = 0.f;
  for (int t = 2; t <= T; ++t) {
    head_prob<CM>(S, bs, t * N + n, oy, ox, Hi, Wi, C, sc);
#pragma unroll
    for (int k = 0; k < CM; ++k) mean[k] += sc[k] - p1[k];
  }
  float sq[CM];
#pragma unroll
  for (int k = 0; k < CM; ++k) {
    mean[k] = mean[k] * invT;
    sq[k] = mean[k] * mean[k];  // sample 1: d_1 = 0
  }
  for (int t = 2; t <= T; ++t) {
    head_prob<CM>(S, bs, t * N + n, oy, ox, Hi, Wi, C, sc);
#pragma unroll
    for (int k = 0; k < CM; ++k) {
      const float d = (sc[k] - p1[k]) - mean[k];
      sq[k] = __builtin_fmaf(d, d, sq[k]);
    }
  }
  float vs = 0.f, mx = 0.f;
#pragma unroll
  for (int k = 0; k < CM; ++k)
    if (k < C) {
      vs += sq[k];
      mx = fmaxf(mx, sq[k]);
    }
  vmax_class = mx * invT;
  return vs * invTC;
}

template <int CM>
__global__ __launch_bounds__(512) void uncertainty_moments_kernel(const float* __restrict__ Sa, const float* __restrict__ Sb,
                                                                 const float* __restrict__ ba, const float* __restrict__ bb,
                                                                 int N, int Hi, int Wi, int C, int T, float* __restrict__ mvar,
                                                                 uint32_t* __restrict__ vmax) {
  __shared__ uint32_t red[8];
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t npix = (int64_t)N * Ho * Wo;
  const int e = blockIdx.y;
  const float* S = e == 0 ? Sa : Sb;
  const float* bs = e == 0 ? ba : bb;
  const float invT = 1.f / (float)T;
  const float invTC = 1.f / (float)(T * C);
  float top = 0.f;
  for (int64_t opix = (int64_t)blockIdx.x * 512 + threadIdx.x; opix < npix; opix += (int64_t)gridDim.x * 512) {
    const int ox = (int)(opix % Wo);
    const int oy = (int)((opix / Wo) % Ho);
    const int n = (int)(opix / ((int64_t)Wo * Ho));
    float vc;
    mvar[(int64_t)e * npix + opix] = head_sample_moments<CM>(S, bs, N, n, oy, ox, Hi, Wi, C, T, invT, invTC, vc);
    top = fmaxf(top, vc);
  }
  xv_block_max_nonneg(top, red, vmax + e);
}

// Fusion head: one output pixel per thread.  Both experts' PLAIN-slot probabilities (head_prob on images 0 .. N-1 of S: the
// bits of decoder_head_kernel's `prob`), mvar and vmax of the moments pass -> xv_udm_mix / xv_udm_add / xv_udm_finish
// (xv_common.h; shared with xv_uncertainty_dirichlet_fuse, which gives the same bits on materialised inputs) -> the label.
// Both experts' parameter tables, their column sums and the log prior sit in LDS.  Optional outputs: fused score
// [N][8Hi][8Wi][C], plain probabilities [2][N][8Hi][8Wi][C], mix [2][N][8Hi][8Wi].
template <int CM>
__global__ __launch_bounds__(256) void uncertainty_dirichlet_head_kernel(
    const float* __restrict__ Sa, const float* __restrict__ Sb, const float* __restrict__ ba, const float* __restrict__ bb, int N,
    int Hi, int Wi, int C, const float* __restrict__ mvar, const float* __restrict__ vmax, const float* __restrict__ A_g,
    const float* __restrict__ logprior, int64_t* __restrict__ label, float* __restrict__ score, float* __restrict__ prob,
    float* __restrict__ mix_out) {
  extern __shared__ __attribute__((aligned(16))) float udm_tab[];  // A [2][C][CM], column sums [2][CM], log prior [CM]
  float* cs = udm_tab + 2 * C * CM;
  float* lp = cs + 2 * CM;
  xv_udm_stage<CM>(udm_tab, cs, A_g, C, threadIdx.x, 256);
  xv_udm_stage<CM>(udm_tab + C * CM, cs + CM, A_g + C * C, C, threadIdx.x, 256);
  if (threadIdx.x < CM) lp[threadIdx.x] = threadIdx.x < C ? logprior[threadIdx.x] : 0.f;
  __syncthreads();
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t npix = (int64_t)N * Ho * Wo;
  const int64_t opix = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (opix >= npix) return;
  const int ox = (int)(opix % Wo);
  const int oy = (int)((opix / Wo) % Ho);
  const int n = (int)(opix / ((int64_t)Wo * Ho));
  float total[CM];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    float sc[CM];
    head_prob<CM>(e == 0 ? Sa : Sb, e == 0 ? ba : bb, n, oy, ox, Hi, Wi, C, sc);
    if (prob) {
      float* dst = prob + ((int64_t)e * npix + opix) * C;
#pragma unroll
      for (int k = 0; k < CM; ++k)
        if (k < C) dst[k] = sc[k];
    }
    const float mix = xv_udm_mix(mvar[(int64_t)e * npix + opix], vmax[e]);
    if (mix_out) mix_out[(int64_t)e * npix + opix] = mix;
    xv_udm_add<CM>(total, sc, mix, udm_tab + e * C * CM, cs + e * CM, C, e == 0);
  }
  label[opix] = xv_udm_finish<CM>(total, lp, C);
  if (score) {
#pragma unroll
    for (int k = 0; k < CM; ++k)
      if (k < C) score[opix * C + k] = total[k];
  }
}

// The Dirichlet form of fused_head_kernel for C == CM on PACKED fp32 (v_pk_mul / v_pk_add / v_pk_fma_f32, two classes per
// instruction): every per-class step of the scalar form that is not a summation chain -- the four-tap interpolation, the bias,
// x - max, the products with log2 e / 1 / sum / ln 2, fma(p, 1 / sum', 1e-20), dot - lognorm, + logprior -- is the same IEEE
// operation on the same operands, so the labels stay those of fused_head_kernel<CM, 1, true> and of the unfused path bit for
// bit; the sums (softmax denominator, renormalisation) keep their order.  P consecutive output pixels ox = P m .. P m + P - 1
// per thread share their taps and every table row read from LDS: the 72 16-byte broadcast reads per pixel of the scalar form
// load the LDS pipe about as long as its instructions load the vector ALU.  16 images of 768x384 (tools/dirichlet_head_ab.py):
// scalar 97-105 us; packed, P = 1: 93-100 (VALU instructions 913 -> 751, the LDS reads as before); P = 2: 82; P = 4: 75 us
// (162 VGPRs, 3 waves per SIMD -- the scalar form with four pixels had measured 14 % SLOWER than with one).
// Other class counts, scalar -> this form: 8: 62-69 -> 45-53 us; 16: 135-141 -> 113-121; 20: 185-191 -> 171-178; 24: 254-259 ->
// 312-314; 32: 396-398 -> 576 (328 / 434 registers): the launcher keeps the scalar form above 20 classes.
template <int CM, int P>
__global__ __launch_bounds__(256) void fused_dirichlet_head_pk_kernel(const float* __restrict__ Sa, const float* __restrict__ Sb,
                                                                     const float* __restrict__ ba, const float* __restrict__ bb,
                                                                     int N, int Hi, int Wi, const float* __restrict__ tab_g,
                                                                     const float* __restrict__ lognorm_g,
                                                                     const float* __restrict__ logprior_g,
                                                                     int64_t* __restrict__ fused) {
  constexpr int H2 = CM / 2;
  extern __shared__ __attribute__((aligned(16))) float tab[];  // [2][CM k][CM c] = alpha_e[c][k] - 1, lognorm [2][CM], logprior [CM]
  float* ln = tab + 2 * CM * CM;
  float* lp = ln + 2 * CM;
  fuse_stage_dirichlet<CM>(tab, ln, tab_g, lognorm_g, 2, CM);
  if (threadIdx.x < CM) lp[threadIdx.x] = logprior_g[threadIdx.x];
  __syncthreads();
  const int Ho = Hi * 8, Wo = Wi * 8, Wq = Wo / P;
  const int64_t nquads = (int64_t)N * Ho * Wq;
  const int64_t quad = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (quad >= nquads) return;
  const int ox0 = (int)(quad % Wq) * P;
  const int oy = (int)((quad / Wq) % Ho);
  const int n = (int)(quad / ((int64_t)Wq * Ho));
  int iy1, ix1;
  float wy1, wy0;
  bilinear_taps<8>(oy, iy1, wy1, wy0);
  {
    float u1, u0;
    bilinear_taps<8>(ox0, ix1, u1, u0);
  }
  f32x2 total[P][H2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
    head_load_taps<CM>(e == 0 ? Sa : Sb, n, iy1, ix1, Hi, Wi, ta, tb, tc, td);
    const float* bs = e == 0 ? ba : bb;
    f32x2 lg[P][H2];  // log(1e-20 + p) of the P pixels
#pragma unroll
    for (int p = 0; p < P; ++p) {
      int ixp;
      float wx1, wx0;
      bilinear_taps<8>(ox0 + p, ixp, wx1, wx0);
      const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
      const f32x2 v00 = f32x2{w00, w00}, v01 = f32x2{w01, w01}, v10 = f32x2{w10, w10}, v11 = f32x2{w11, w11};
      f32x2 s[H2];
#pragma unroll
      for (int j = 0; j < H2; ++j) {  // head_eval_taps: fmaf(d, w11, fmaf(c, w10, fmaf(b, w01, a * w00))) + bias
        const int k4 = j >> 1;
        const f32x2 a2 = (j & 1) ? f32x2{ta[k4].z, ta[k4].w} : f32x2{ta[k4].x, ta[k4].y};
        const f32x2 b2 = (j & 1) ? f32x2{tb[k4].z, tb[k4].w} : f32x2{tb[k4].x, tb[k4].y};
        const f32x2 c2 = (j & 1) ? f32x2{tc[k4].z, tc[k4].w} : f32x2{tc[k4].x, tc[k4].y};
        const f32x2 d2 = (j & 1) ? f32x2{td[k4].z, td[k4].w} : f32x2{td[k4].x, td[k4].y};
        f32x2 t = a2 * v00;
        t = __builtin_elementwise_fma(b2, v01, t);
        t = __builtin_elementwise_fma(c2, v10, t);
        t = __builtin_elementwise_fma(d2, v11, t);
        const f32x2 bias2 = f32x2{bs[2 * j], bs[2 * j + 1]};
        s[j] = t + bias2;
      }
      float m = s[0].x;  // head_max
#pragma unroll
      for (int j = 0; j < H2; ++j) {
        if (j) m = fmaxf(m, s[j].x);
        m = fmaxf(m, s[j].y);
      }
      const f32x2 m2 = f32x2{m, m};
      float sum = 0.f;  // head_softmax: exp(x - max) / sum
#pragma unroll
      for (int j = 0; j < H2; ++j) {
        f32x2 t = s[j] - m2;
        t = t * f32x2{1.4426950408889634f, 1.4426950408889634f};
        s[j] = f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
        sum += s[j].x;
        sum += s[j].y;
      }
      const float rsum = xv_fast_rcp(sum);
      const f32x2 rsum2 = f32x2{rsum, rsum};
      float sum1 = 0.f;  // the probabilities the unfused path stores, renormalised, log(1e-20 + p)
#pragma unroll
      for (int j = 0; j < H2; ++j) {
        s[j] = s[j] * rsum2;
        sum1 += s[j].x;
        sum1 += s[j].y;
      }
      const float rs = xv_fast_rcp(sum1);
      const f32x2 rs2 = f32x2{rs, rs};
#pragma unroll
      for (int j = 0; j < H2; ++j) {
        const f32x2 t = __builtin_elementwise_fma(s[j], rs2, f32x2{1e-20f, 1e-20f});
        const f32x2 l = f32x2{__builtin_amdgcn_logf(t.x), __builtin_amdgcn_logf(t.y)};
        lg[p][j] = l * f32x2{0.6931471805599453f, 0.6931471805599453f};
      }
    }
    // sum_k (alpha[c][k] - 1) log p[k]: the fmaf chain over k of dirichlet_fuse_kernel, two classes per v_pk_fma_f32
    f32x2 dot[P][H2];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int cp = 0; cp < H2; ++cp) dot[p][cp] = f32x2{0.f, 0.f};
#pragma unroll
    for (int k = 0; k < CM; ++k) {
      const f32x2* rowk = reinterpret_cast<const f32x2*>(tab + (e * CM + k) * CM);
#pragma unroll
      for (int cp = 0; cp < H2; ++cp) {
        const f32x2 r = rowk[cp];
#pragma unroll
        for (int p = 0; p < P; ++p) {
          const float lk = lg[p][k >> 1][k & 1];
          dot[p][cp] = __builtin_elementwise_fma(r, f32x2{lk, lk}, dot[p][cp]);
        }
      }
    }
    const f32x2* ln2 = reinterpret_cast<const f32x2*>(ln + e * CM);
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int cp = 0; cp < H2; ++cp) {
        const f32x2 L = dot[p][cp] - ln2[cp];
        total[p][cp] = e == 0 ? L : total[p][cp] + L;
      }
  }
  const f32x2* lp2 = reinterpret_cast<const f32x2*>(lp);
  int64_t out[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    float best = 0.f;
    int bi = 0;
#pragma unroll
    for (int j = 0; j < H2; ++j) {
      const f32x2 v = total[p][j] + lp2[j];
      if (j == 0 || v.x > best) best = v.x, bi = 2 * j;
      if (v.y > best) best = v.y, bi = 2 * j + 1;
    }
    out[p] = bi;
  }
  int64_t* dst = fused + quad * P;
  if constexpr (P % 2 == 0) {
    typedef __attribute__((ext_vector_type(2))) long long i64x2;
#pragma unroll
    for (int p = 0; p < P; p += 2) *reinterpret_cast<i64x2*>(dst + p) = i64x2{out[p], out[p + 1]};
  } else {
#pragma unroll
    for (int p = 0; p < P; ++p) dst[p] = out[p];
  }
}

// ---- grid-scoring heads (experiments/different_evaluation_parameters.py:10-61: one evaluate() per grid point) --------------
// The searched fusion parameters (sigma, class_prior, delta, beta) never reach the trunks: they only change the small tables
// the fused head reads.  So the trunks run once per batch and these kernels score every pixel under ALL parameter sets, counting
// straight into confusion matrices in LDS: no label map, probability map or per-point intermediate reaches HBM.
//
// Equal keys of a wave are aggregated before they reach the LDS counters: xv_wave_count (xv_heads.h).

// Dirichlet: per pixel ONCE both experts' log(1e-20 + p) -- head_load_taps / head_eval_taps / head_max / head_softmax /
// fuse_renorm_log, as fused_head_kernel<CM, 1> -- then per grid point g its dot products four classes at a time (the
// ascending-k fma chain of dirichlet_fuse_kernel, written out: xv_fuse.h says why), - lognorm, expert 0 + expert 1, + logprior,
// first maximum: the label xv_fused_head_fwd gives with point g's tables, bit for bit.  cm[g][label][pred] += 1 for the pixels
// xv_confusion_matrix counts (0 <= label < C).  LDS: per point the tables [2][CM k][CM c], lognorm [2][CM], logprior [CM], then
// u32 counters [G][C][C].  A bounded grid, pixels in a grid-stride loop
// whose trip count is uniform over the workgroup (xv_wave_count needs whole waves; a lane past the end recomputes the last
// pixel and counts nothing), one 64-bit global atomic per non-zero cell and workgroup.
template <int CM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CM <= 16 ? 4 : 1))) void fused_head_grid_score_kernel(const float* __restrict__ Sa, const float* __restrict__ Sb,
                                                                   const float* __restrict__ ba, const float* __restrict__ bb,
                                                                   int N, int Hi, int Wi, int C, int G,
                                                                   const float* __restrict__ tab_g,
                                                                   const float* __restrict__ lognorm_g,
                                                                   const float* __restrict__ logprior_g,
                                                                   const int32_t* __restrict__ labels,
                                                                   unsigned long long* __restrict__ cm) {
  constexpr int PT = 2 * CM * CM + 3 * CM;  // floats per grid point
  extern __shared__ __attribute__((aligned(16))) float gs_tab[];
  uint32_t* cnt = reinterpret_cast<uint32_t*>(gs_tab + G * PT);
  fuse_stage_dirichlet_points<CM>(gs_tab, tab_g, lognorm_g, logprior_g, 2, G, C);
  for (int i = threadIdx.x; i < G * C * C; i += 256) cnt[i] = 0u;
  __syncthreads();
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t npix = (int64_t)N * Ho * Wo;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < npix; base += (int64_t)gridDim.x * 256) {
    const bool live = base + threadIdx.x < npix;
    if (__ballot(live) == 0) continue;  // (wave-uniform)
    const int64_t opix = live ? base + threadIdx.x : npix - 1;
    const int ox = (int)(opix % Wo);
    const int oy = (int)((opix / Wo) % Ho);
    const int n = (int)(opix / ((int64_t)Wo * Ho));
    int iy1, ix1;
    float wy1, wy0, wx1, wx0;
    bilinear_taps<8>(oy, iy1, wy1, wy0);
    bilinear_taps<8>(ox, ix1, wx1, wx0);
    f32x2 lg[2][CM / 2];  // log(1e-20 + p) of both experts, class pairs (the splat of one class is an operand modifier)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      // the second expert's taps are requested after the first one's arithmetic (its address waits for a result of it: an
      // empty asm, no instruction): both sets of taps at once are 8 CM registers, and the scheduler does ask for them together
      int ne = n;
      if (e == 1) asm volatile("" : "+v"(ne) : "v"(lg[0][CM / 2 - 1].y));
      f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
      head_load_taps<CM>(e == 0 ? Sa : Sb, ne, iy1, ix1, Hi, Wi, ta, tb, tc, td);
      float sc[CM];
      head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, e == 0 ? ba : bb, C, sc);
      const float m = head_max<CM>(sc, C);
      head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
      fuse_renorm_log<CM, true>(sc, C);
#pragma unroll
      for (int k2 = 0; k2 < CM / 2; ++k2) lg[e][k2] = f32x2{sc[2 * k2], sc[2 * k2 + 1]};
    }
    const int l = live ? labels[opix] : -1;
    const bool valid = l >= 0 && l < C;
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      const float* tg = gs_tab + g * PT;
      const float* ln = tg + 2 * CM * CM;
      const float* lp = ln + 2 * CM;
      // four classes at a time, both experts' dot products side by side: nothing of size CM but lg stays live
      float best = 0.f;
      int bi = 0;
#pragma unroll
      for (int c4 = 0; c4 < CM / 4; ++c4) {
        f32x2 dot2[2][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          dot2[e][0] = dot2[e][1] = f32x2{0.f, 0.f};
#pragma unroll
          for (int k = 0; k < CM; ++k) {
            const f32x4 r = *reinterpret_cast<const f32x4*>(tg + (e * CM + k) * CM + 4 * c4);
            const f32x2 lk = (k & 1) ? lg[e][k >> 1].yy : lg[e][k >> 1].xx;
            dot2[e][0] = __builtin_elementwise_fma(f32x2{r.x, r.y}, lk, dot2[e][0]);
            dot2[e][1] = __builtin_elementwise_fma(f32x2{r.z, r.w}, lk, dot2[e][1]);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = 4 * c4 + j;
          const float L0 = dot2[0][j >> 1][j & 1] - ln[c];
          const float L1 = dot2[1][j >> 1][j & 1] - ln[CM + c];
          const float total = L0 + L1;
          const float v = total + lp[c];
          if (c < C && (c == 0 || v > best)) {
            best = v;
            bi = c;
          }
        }
      }
      xv_wave_count(cnt + g * C * C, valid ? l * C + bi : -1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < G * C * C; i += 256) {
    const uint32_t v = cnt[i];
    if (v) atomicAdd(&cm[i], (unsigned long long)v);
  }
}

// Bayes: a fused label is a function of the two experts' labels alone, so ONE joint histogram hist[label][a][b] gives every
// grid point's confusion matrix on the host (cm_g[l][dec_g[a][b]] += hist[l][a][b]); its marginals are the experts' own
// matrices.  The experts' labels as in fused_head_kernel<CM, 0>: head_label_fast, head_softmax when it returns -1, P
// consecutive output pixels per thread on shared taps: four up to 12 classes, two above (four pixels' scores beside the 4 CM
// registers of the taps leave the four waves per SIMD at 16 classes).  u32 counters [C][C][C] in LDS (32 KB at 20 classes), the
// grid and the flush of the kernel above.
template <int CM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CM <= 16 ? 4 : 1))) void fused_head_joint_hist_kernel(const float* __restrict__ Sa, const float* __restrict__ Sb,
                                                                   const float* __restrict__ ba, const float* __restrict__ bb,
                                                                   int N, int Hi, int Wi, int C,
                                                                   const int32_t* __restrict__ labels,
                                                                   unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t jh_cnt[];  // [C][C][C]
  const int cells = C * C * C;
  for (int i = threadIdx.x; i < cells; i += 256) jh_cnt[i] = 0u;
  __syncthreads();
  constexpr int P = xv_joint_hist_pixels(CM);
  const int Ho = Hi * 8, Wo = Wi * 8, Wq = Wo / P;
  const int64_t nquads = (int64_t)N * Ho * Wq;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < nquads; base += (int64_t)gridDim.x * 256) {
    const bool live = base + threadIdx.x < nquads;
    if (__ballot(live) == 0) continue;  // (wave-uniform)
    const int64_t quad = live ? base + threadIdx.x : nquads - 1;
    const int ox0 = (int)(quad % Wq) * P;
    const int oy = (int)((quad / Wq) % Ho);
    const int n = (int)(quad / ((int64_t)Wq * Ho));
    int iy1, ix1;
    float wy1, wy0;
    bilinear_taps<8>(oy, iy1, wy1, wy0);
    {
      float u1, u0;
      bilinear_taps<8>(ox0, ix1, u1, u0);
    }
    int lab[2][P];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      // (the second expert's taps wait for the first one's labels, as in the kernel above)
      int ne = n;
      if (e == 1) asm volatile("" : "+v"(ne) : "v"(lab[0][P - 1]));
      f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
      head_load_taps<CM>(e == 0 ? Sa : Sb, ne, iy1, ix1, Hi, Wi, ta, tb, tc, td);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        int ixp;
        float wx1, wx0;
        bilinear_taps<8>(ox0 + p, ixp, wx1, wx0);
        float sc[CM];
        head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, e == 0 ? ba : bb, C, sc);
        const float m = head_max<CM>(sc, C);
        int l = head_label_fast<CM>(sc, m, C);
        if (l < 0) l = head_softmax<CM>(sc, m, C);
        lab[e][p] = l;
      }
    }
    typedef int i32xP __attribute__((ext_vector_type(P)));
    const i32xP lv = *reinterpret_cast<const i32xP*>(labels + quad * P);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int l = lv[p];
      xv_wave_count(jh_cnt, (live && l >= 0 && l < C) ? (l * C + lab[0][p]) * C + lab[1][p] : -1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += 256) {
    const uint32_t v = jh_cnt[i];
    if (v) atomicAdd(&hist[i], (unsigned long long)v);
  }
}

// ---- fused average head (average_mix.py:18-21 on the low-resolution class scores) ------------------------------------------
// Both experts' probabilities per output pixel -- head_load_taps / head_eval_taps / head_max / head_softmax: the bits
// decoder_head_kernel stores as `prob` -- then average_fuse_kernel's (fusion.hip) statements for two experts: s[k] = pa[k] +
// pb[k], v = s[k] / 2, first-maximum argmax over k < C.  The labels are those of two decoder heads with `prob` + xv_average_fuse
// bit for bit, and the two float32 probability maps (2 x 4C bytes per pixel, written and read back) never exist.
// P = TWO consecutive output pixels per thread on shared taps: a thread holds the 4 CM registers of one expert's taps, the
// first expert's P CM probabilities and the CM values of the pixel in work, (5 + P) CM in all -- four pixels as in the Bayes
// head are 108 registers at 12 classes before any address or weight.  The pixels of a group and the two experts are worked
// through one after the other (empty asm statements that make the next one's input wait for the last result, no instruction):
// left alone the scheduler interleaves them and every interleaved pixel adds CM live registers (12 classes: 128 registers and
// 68 to 100 bytes of scratch in the counting form).  At 16 classes 7 CM = 112 registers still leave nothing for the rest, so
// there the first expert's probabilities wait in LDS (a private 16-byte column per thread and class quad, no barrier).
// COUNT = false: the label map int64 [N][8Hi][8Wi], one 16-byte store per thread; a grid that covers every pixel group (one
// trip of the loop).  COUNT = true: cm[label][fused] += 1 over the pixels with 0 <= label < C and no label map: u32 counters
// [C][C] in LDS through xv_wave_count, a bounded grid with a grid-stride loop whose trip count is uniform over the workgroup
// (a lane past the end recomputes the last group and counts nothing), one 64-bit global atomic per non-zero cell and
// workgroup -- the scheme of fused_head_joint_hist_kernel.  FULL: the class count IS CM, every `k < C` folds away.
constexpr int XV_AVERAGE_PIXELS = 2;
constexpr bool xv_average_stash(int cm) { return cm == 16; }
// dynamic LDS of one launch: the counters (counting form), then the stash
static size_t average_head_lds(int num_classes, bool count) {
  const int cm = (num_classes + 3) / 4 * 4;
  return (count ? (size_t)(num_classes * num_classes + 3) / 4 * 16 : 0) +
         (xv_average_stash(cm) ? (size_t)256 * XV_AVERAGE_PIXELS * cm * 4 : 0);
}

template <int CM, bool COUNT, bool FULL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CM <= 16 ? 4 : 1))) void fused_head_average_kernel(
    const float* __restrict__ Sa, const float* __restrict__ Sb, const float* __restrict__ ba, const float* __restrict__ bb, int N,
    int Hi, int Wi, int C_, int64_t* __restrict__ fused, const int32_t* __restrict__ labels,
    unsigned long long* __restrict__ cm) {
  const int C = FULL ? CM : C_;
  constexpr int P = XV_AVERAGE_PIXELS;
  constexpr bool STASH = xv_average_stash(CM);
  constexpr int SR = STASH ? 1 : P;  // rows of the first expert's probabilities kept in registers
  static_assert(8 % P == 0 && P % 2 == 0, "a pixel group is whole 16-byte stores inside one source column");
  extern __shared__ __attribute__((aligned(16))) uint32_t av_cnt[];  // COUNT: [C][C]; STASH: f32x4 [P][CM / 4][256] behind it
  f32x4* stash = reinterpret_cast<f32x4*>(av_cnt + (COUNT ? (C * C + 3) / 4 * 4 : 0)) + threadIdx.x;
  if constexpr (COUNT) {
    for (int i = threadIdx.x; i < C * C; i += 256) av_cnt[i] = 0u;
    __syncthreads();
  }
  const int Ho = Hi * 8, Wo = Wi * 8, Wq = Wo / P;
  const int64_t nquads = (int64_t)N * Ho * Wq;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < nquads; base += (int64_t)gridDim.x * 256) {
    const bool live = base + threadIdx.x < nquads;
    if (__ballot(live) == 0) continue;  // (wave-uniform)
    const int64_t quad = live ? base + threadIdx.x : nquads - 1;
    const int ox0 = (int)(quad % Wq) * P;
    const int oy = (int)((quad / Wq) % Ho);
    const int n = (int)(quad / ((int64_t)Wq * Ho));
    int iy1, ix1;
    float wy1, wy0;
    bilinear_taps<8>(oy, iy1, wy1, wy0);
    {
      float u1, u0;
      bilinear_taps<8>(ox0, ix1, u1, u0);
    }
    float pa[SR][CM];  // the first expert's probabilities (STASH: of the pixel in work)
    int out[P];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      int ne = n;
      if (e == 1) asm volatile("" : "+v"(ne) : "v"(pa[SR - 1][CM - 1]));
      f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
      head_load_taps<CM>(e == 0 ? Sa : Sb, ne, iy1, ix1, Hi, Wi, ta, tb, tc, td);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int r = STASH ? 0 : p;
        int ixp;
        float wx1, wx0;
        bilinear_taps<8>(ox0 + p, ixp, wx1, wx0);
        if (p > 0) {
          if (e == 0)
            asm volatile("" : "+v"(wx1) : "v"(pa[STASH ? 0 : p - 1][CM - 1]));
          else
            asm volatile("" : "+v"(wx1) : "v"(out[p - 1]));
        }
        float sc[CM];
        head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, e == 0 ? ba : bb, C, sc);
        const float m = head_max<CM>(sc, C);
        head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
        if (e == 0) {
#pragma unroll
          for (int k = 0; k < CM; ++k) pa[r][k] = sc[k];
          if constexpr (STASH) {
#pragma unroll
            for (int k4 = 0; k4 < CM / 4; ++k4)
              stash[(p * (CM / 4) + k4) * 256] = f32x4{sc[4 * k4], sc[4 * k4 + 1], sc[4 * k4 + 2], sc[4 * k4 + 3]};
          }
        } else {
          if constexpr (STASH) {
#pragma unroll
            for (int k4 = 0; k4 < CM / 4; ++k4) {
              const f32x4 t = stash[(p * (CM / 4) + k4) * 256];
              pa[0][4 * k4] = t.x, pa[0][4 * k4 + 1] = t.y, pa[0][4 * k4 + 2] = t.z, pa[0][4 * k4 + 3] = t.w;
            }
          }
          // average_fuse_kernel for two experts: s = pa + pb, v = s / 2, the first maximum
          float best = 0.f;
          int bi = 0;
#pragma unroll
          for (int k = 0; k < CM; ++k) {
            const float s = pa[r][k] + sc[k];
            const float v = s / 2.0f;
            if (k < C && (k == 0 || v > best)) {
              best = v;
              bi = k;
            }
          }
          out[p] = bi;
        }
      }
    }
    if constexpr (COUNT) {
      typedef int i32xP __attribute__((ext_vector_type(P)));
      const i32xP lv = *reinterpret_cast<const i32xP*>(labels + quad * P);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int l = lv[p];
        xv_wave_count(av_cnt, (live && l >= 0 && l < C) ? l * C + out[p] : -1);
      }
    } else if (live) {
      typedef __attribute__((ext_vector_type(2))) long long i64x2;
      int64_t* dst = fused + quad * P;
#pragma unroll
      for (int p = 0; p < P; p += 2) *reinterpret_cast<i64x2*>(dst + p) = i64x2{out[p], out[p + 1]};
    }
  }
  if constexpr (COUNT) {
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256) {
      const uint32_t v = av_cnt[i];
      if (v) atomicAdd(&cm[i], (unsigned long long)v);
    }
  }
}

// ---- fused head for two to four experts (bayes_mix.py:33-58, dirichlet_mix.py:14-36,96-136, average_mix.py:18-21) ------------
// fused_head_kernel / fused_head_average_kernel generalised from two experts to E = 2 .. 4: per output pixel and expert
// head_load_taps / head_eval_taps / head_max, then head_label_fast + head_softmax (MODE 0) or head_softmax (MODE 1, 2) -- each
// expert's label / probabilities with the bits decoder_head_kernel stores -- then the fusion of xv_fuse.h, the experts in
// ascending order:
//   MODE 0, Bayes      score[k] = ((tab_0[l_0][k] + tab_1[l_1][k]) + ...) + logprior[k], written out   (bayes_fuse_kernel)
//   MODE 1, Dirichlet  fused_head_kernel<CM, 1>'s statements (written out), fuse_argmax_prior       (dirichlet_fuse_kernel)
//   MODE 2, mean       s = ((p_0 + p_1) + ...), fuse_argmax_mean                                    (average_fuse_kernel)
// The labels are those of E decoder heads + xv_bayes_fuse / xv_dirichlet_fuse / xv_average_fuse bit for
// bit; the E label maps or probability maps between them never exist.  The experts are worked one after another in a loop
// that is NOT unrolled into the running registers (Bayes: the labels of a pixel packed into one word; Dirichlet: total [CM];
// mean: s [P][CM]): nothing of size E * C is held, and the register count is the two-expert sibling's whatever E is.  The score
// and bias pointers are kernel arguments (HeadPtrs, as LabelPtrs / ProbPtrs in fusion.hip): no pointer table in device
// memory, a captured graph of the step stays valid.
// Pixels per thread as the siblings: Bayes four (two 16-byte stores), Dirichlet one (the scalar form of fused_head_kernel with
// its v_pk_fma_f32 dot products), mean two (one 16-byte store).
// Bayes decides through a table dec [C^E] (one byte per entry) built by the workgroup where C^E <= XV_MULTI_DEC_MAX, and sums
// the E table rows per pixel above it.  The table pays for itself only while building it is cheaper than what it saves: an
// entry costs what the per-pixel sum of one pixel costs (E row reads, E C adds, a C-way argmax), a workgroup has 1 024 pixels,
// so 1 024 entries (four per thread) is where the table stops winning: two experts at any class count, three up to 10
// classes, four up to 5.  Either way the sums and their order are bayes_fuse_kernel's.
// LDS: tab [E][C][CM] (Dirichlet: transposed [E][CM k][CM c]), lognorm [E][CM], logprior [CM], dec.
// (XV_MULTI_MAXE, HeadPtrs and head_ptr: xv_heads.h, shared with the counting form in multi_count.hip)
constexpr int XV_MULTI_DEC_MAX = 1024;

constexpr int xv_multi_pixels(int mode) { return mode == 0 ? 4 : (mode == 1 ? 1 : 2); }

static int multi_head_dec_entries(int num_classes, int num_experts) {
  int64_t nd = 1;
  for (int e = 0; e < num_experts; ++e) nd *= num_classes;
  return nd <= XV_MULTI_DEC_MAX ? (int)nd : 0;
}

// waves per SIMD the register allocation is held to: at 12 classes what the two-expert siblings reach (Bayes and mean four,
// Dirichlet eight with the class count folded and seven without); the wide Dirichlet forms are named too, because left alone
// the compiler keeps table rows of the rolled expert loop in registers (16 classes, run-time count: 286 registers)
constexpr int xv_multi_waves(int cm, int mode, bool full) {
  if (mode != 1) return cm <= 12 ? 4 : 1;
  return cm <= 8 ? 8 : (cm == 12 ? (full ? 8 : 7) : (cm <= 24 ? 4 : 3));
}

template <int CM, int MODE, bool FULL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(xv_multi_waves(CM, MODE, FULL)))) void fused_head_multi_kernel(
    HeadPtrs ptrs, int E, int N, int Hi, int Wi, int C_, int ndec, const float* __restrict__ tab_g,
    const float* __restrict__ lognorm_g, const float* __restrict__ logprior_g, int64_t* __restrict__ fused) {
  const int C = FULL ? CM : C_;
  constexpr int P = xv_multi_pixels(MODE);
  extern __shared__ __attribute__((aligned(16))) float tab[];
  const int rows = MODE == 1 ? CM : C;  // table rows per expert
  float* ln = tab + E * rows * CM;
  float* lp = ln + E * CM;
  uint8_t* dec = reinterpret_cast<uint8_t*>(lp + CM);  // [ndec]
  if constexpr (MODE == 1) fuse_stage_dirichlet<CM>(tab, ln, tab_g, lognorm_g, E, C);
  if constexpr (MODE == 0) {
    for (int i = threadIdx.x; i < E * C * CM; i += 256) {
      const int k = i % CM, row = i / CM;
      tab[i] = k < C ? tab_g[row * C + k] : 0.f;
    }
  }
  if constexpr (MODE != 2) {
    if (threadIdx.x < CM) lp[threadIdx.x] = threadIdx.x < C ? logprior_g[threadIdx.x] : 0.f;
    __syncthreads();
  }
  if constexpr (MODE == 0) {
    // dec[((l_0 C + l_1) C + ...) + l_{E-1}] = the label bayes_fuse_kernel gives these expert labels
    if (ndec > 0) {
      for (int i = threadIdx.x; i < ndec; i += 256) {
        int l[XV_MULTI_MAXE], r = i;
#pragma unroll
        for (int e = XV_MULTI_MAXE - 1; e >= 0; --e) {
          l[e] = 0;
          if (e < E) {
            l[e] = r % C;
            r = r / C;
          }
        }
        float best = 0.f;
        int bi = 0;
        for (int k = 0; k < C; ++k) {
          float sc = tab[l[0] * CM + k];
#pragma unroll
          for (int e = 1; e < XV_MULTI_MAXE; ++e)
            if (e < E) sc = sc + tab[(e * C + l[e]) * CM + k];
          const float v = sc + lp[k];
          if (k == 0 || v > best) {
            best = v;
            bi = k;
          }
        }
        dec[i] = (uint8_t)bi;
      }
      __syncthreads();
    }
  }
  const int Ho = Hi * 8, Wo = Wi * 8, Wq = Wo / P;
  const int64_t nquads = (int64_t)N * Ho * Wq;
  const int64_t quad = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (quad >= nquads) return;
  const int ox0 = (int)(quad % Wq) * P;
  const int oy = (int)((quad / Wq) % Ho);
  const int n = (int)(quad / ((int64_t)Wq * Ho));
  int iy1, ix1;
  float wy1, wy0;
  bilinear_taps<8>(oy, iy1, wy1, wy0);
  {
    float u1, u0;
    bilinear_taps<8>(ox0, ix1, u1, u0);
  }
  // running state over the experts.  Bayes: the pixel's expert labels in one word, l_0 first: radix C where the table decides
  // (the word IS the table index), 5 bits each where the rows are summed
  constexpr int NT = MODE == 0 ? 1 : CM;
  float total[P][NT];
  int key[P];
  const int radix = ndec > 0 ? C : 32;
#pragma unroll
  for (int p = 0; p < P; ++p) key[p] = 0;
#pragma nounroll
  for (int e = 0; e < E; ++e) {
    const float* S = head_ptr(ptrs.s, e);
    const float* bs = head_ptr(ptrs.b, e);
    f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
    head_load_taps<CM>(S, n, iy1, ix1, Hi, Wi, ta, tb, tc, td);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      int ixp;
      float wx1, wx0;
      bilinear_taps<8>(ox0 + p, ixp, wx1, wx0);
      if constexpr (MODE == 2) {
        // one pixel after the other: left alone the scheduler interleaves them and each adds CM live registers (see
        // fused_head_average_kernel); no instruction
        if (p > 0) asm volatile("" : "+v"(wx1) : "v"(total[p - 1][CM - 1]));
      }
      float sc[CM];
      head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, bs, C, sc);
      const float m = head_max<CM>(sc, C);
      if constexpr (MODE == 0) {
        int l = head_label_fast<CM>(sc, m, C);
        if (l < 0) l = head_softmax<CM>(sc, m, C);
        key[p] = key[p] * radix + l;
      } else if constexpr (MODE == 2) {
        head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
#pragma unroll
        for (int k = 0; k < CM; ++k) total[p][k] = e == 0 ? sc[k] : total[p][k] + sc[k];
      } else {
        head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
        float sum = 0.f;  // (fuse_renorm_log of xv_fuse.h, written out: through it this kernel measured slower, see there)
#pragma unroll
        for (int k = 0; k < CM; ++k) {
          sc[k] = k < C ? sc[k] : 0.f;
          sum += sc[k];
        }
        const float rs = xv_fast_rcp(sum);
#pragma unroll
        for (int k = 0; k < CM; ++k) sc[k] = k < C ? xv_fast_log(1e-20f + sc[k] * rs) : 0.f;  // renormalise, then log(1e-20 + p)
        // the fmaf chain over k of dirichlet_fuse_kernel per class, two classes per v_pk_fma_f32 on the transposed table
        // (padded classes / terms are exact zeros: fma(0, 0, d) = d), as fused_head_kernel
        f32x2 dot2[CM / 2];
#pragma unroll
        for (int cp = 0; cp < CM / 2; ++cp) dot2[cp] = f32x2{0.f, 0.f};
#pragma unroll
        for (int k = 0; k < CM; ++k) {
          const f32x2* rowk = reinterpret_cast<const f32x2*>(tab + (e * CM + k) * CM);
          const f32x2 lk = f32x2{sc[k], sc[k]};
#pragma unroll
          for (int cp = 0; cp < CM / 2; ++cp) dot2[cp] = __builtin_elementwise_fma(rowk[cp], lk, dot2[cp]);
        }
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          const float L = dot2[c >> 1][c & 1] - ln[e * CM + c];
          total[p][c] = c < C ? (e == 0 ? L : total[p][c] + L) : 0.f;
        }
      }
    }
  }
  int64_t out[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    float best = 0.f;
    int bi = 0;
    if constexpr (MODE == 0) {
      if (ndec > 0) {
        bi = dec[key[p]];
      } else {
        // bayes_fuse_kernel: the E rows of the pixel's labels summed in ascending expert order
        float sc[CM];
#pragma nounroll
        for (int e = 0; e < E; ++e) {
          const int l = (key[p] >> (5 * (E - 1 - e))) & 31;
          const f32x4* row = reinterpret_cast<const f32x4*>(tab + (e * C + l) * CM);
#pragma unroll
          for (int k4 = 0; k4 < CM / 4; ++k4) {
            const f32x4 r = row[k4];
            sc[4 * k4] = e == 0 ? r.x : sc[4 * k4] + r.x;
            sc[4 * k4 + 1] = e == 0 ? r.y : sc[4 * k4 + 1] + r.y;
            sc[4 * k4 + 2] = e == 0 ? r.z : sc[4 * k4 + 2] + r.z;
            sc[4 * k4 + 3] = e == 0 ? r.w : sc[4 * k4 + 3] + r.w;
          }
        }
#pragma unroll
        for (int k = 0; k < CM; ++k) {
          const float v = sc[k] + lp[k];
          if (k < C && (k == 0 || v > best)) {
            best = v;
            bi = k;
          }
        }
      }
    } else if constexpr (MODE == 1) {
      bi = fuse_argmax_prior<CM>(total[p], lp, C);
    } else {
      bi = fuse_argmax_mean<CM>(total[p], (float)E, C);
    }
    (void)best;
    out[p] = bi;
  }
  int64_t* dst = fused + quad * P;
  if constexpr (P % 2 == 0) {
    typedef __attribute__((ext_vector_type(2))) long long i64x2;
#pragma unroll
    for (int p = 0; p < P; p += 2) *reinterpret_cast<i64x2*>(dst + p) = i64x2{out[p], out[p + 1]};
  } else {
#pragma unroll
    for (int p = 0; p < P; ++p) dst[p] = out[p];
  }
}

// ---- softmax + argmax on dense fp32 scores (basic_fusion_model.py:21-22) -------------------------
template <int CMAX>
__global__ __launch_bounds__(256) void softmax_argmax_kernel(const float* __restrict__ score, int64_t npix, int C,
                                                            float* __restrict__ prob, int64_t* __restrict__ label) {
  for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += (int64_t)gridDim.x * 256) {
    float sc[CMAX];
    // C == CMAX (a multiple of 4: the 12 classes of the headline model): a pixel's scores / probabilities are whole 16-byte
    // vectors (4-byte accesses at a 48-byte lane stride ran at 0.26 of the HBM rate)
    const bool vec = C == CMAX && (CMAX & 3) == 0 && CMAX != 16 && CMAX != 32;  // (the 16 / 32 forms take unaligned pointers)
    if (vec) {
#pragma unroll
      for (int q = 0; q < CMAX / 4; ++q) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(score + pix * CMAX + 4 * q);
        sc[4 * q] = t.x, sc[4 * q + 1] = t.y, sc[4 * q + 2] = t.z, sc[4 * q + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < CMAX; ++k) sc[k] = k < C ? score[pix * C + k] : 0.f;
    }
    float m = sc[0];
#pragma unroll
    for (int k = 1; k < CMAX; ++k)
      if (k < C) m = fmaxf(m, sc[k]);
    float e[CMAX];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CMAX; ++k) {
      e[k] = k < C ? xv_fast_exp(sc[k] - m) : 0.f;
      sum += e[k];
    }
    const float rsum = xv_fast_rcp(sum);
    float best = -1.f;
    int bi = 0;
#pragma unroll
    for (int k = 0; k < CMAX; ++k) {
      const float p = e[k] * rsum;
      e[k] = p;
      if (k < C) {
        if (prob && !vec) prob[pix * C + k] = p;
        if (p > best) {
          best = p;
          bi = k;
        }
      }
    }
    if (prob && vec) {
#pragma unroll
      for (int q = 0; q < CMAX / 4; ++q)
        *reinterpret_cast<f32x4*>(prob + pix * CMAX + 4 * q) = f32x4{e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]};
    }
    if (label) label[pix] = bi;
  }
}

// ---- general decoder head: bilinear x8 -> per-channel affine (inference batch norm) -> relu -> 1x1 score ->
// softmax -> argmax, un-commuted.  The default head (score_lowres + decoder_head_kernel) moves the 1x1 conv in
// front of the interpolation, which is only valid while relu(up8(f)) == up8(f); a batch norm with a non-zero shift
// between the deconv and its relu (custom_layers.py:112-119, the default of decoder() when fusion_fcn.py:38
// calls it) breaks that, and this kernel interpolates all U features per pixel instead (16x the FMAs).
// One thread = 4 horizontally consecutive output pixels sharing the same 2x2 source pixels.
template <int CM, bool CLAMP>
__device__ inline void head_affine_group(const u32x4& a00, const u32x4& a01, const u32x4& a10, const u32x4& a11, float wy0,
                                  float wy1, const float (&wx0)[4], const float (&wx1)[4],
                                  const float* __restrict__ wrow, const float* __restrict__ srow,
                                  const float* __restrict__ trow, int C, int remain, float (&sc)[4][CM]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int sh = (i & 1) * 16, q = i >> 1;
    const float f00 = bf16_bits_to_f32((a00[q] >> sh) & 0xffffu), f01 = bf16_bits_to_f32((a01[q] >> sh) & 0xffffu);
    const float f10 = bf16_bits_to_f32((a10[q] >> sh) & 0xffffu), f11 = bf16_bits_to_f32((a11[q] >> sh) & 0xffffu);
    const float v0 = f00 * wy0 + f10 * wy1;  // source column ix0
    const float v1 = f01 * wy0 + f11 * wy1;  // source column ix1
    float up[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) up[j] = fmaxf((v0 * wx0[j] + v1 * wx1[j]) * srow[i] + trow[i], 0.f);
    if (CLAMP && i * C + CM > remain) {  // wave-uniform
#pragma unroll
      for (int k = 0; k < CM; ++k) {
        int off = i * C + k;
        off = off < remain ? off : remain - 1;
        const float wv = wrow[off];
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j][k] = fmaf(up[j], wv, sc[j][k]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < CM; ++k) {
        const float wv = wrow[i * C + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) sc[j][k] = fmaf(up[j], wv, sc[j][k]);
      }
    }
  }
}

template <int CM>
__global__ __launch_bounds__(256) void decoder_head_affine_kernel(const __bf16* __restrict__ f, const float* __restrict__ sc_g,
                                                                 const float* __restrict__ sh_g, const float* __restrict__ ws_g,
                                                          const float* __restrict__ bs_g, int N, int Hi, int Wi, int U,
                                                          int C, float* __restrict__ score, float* __restrict__ prob,
                                                          int64_t* __restrict__ label) {
  const int Ho = Hi * 8, Wo = Wi * 8;
  // block = 128 x 8 output pixels: a wave covers 2 rows x 128 columns
  const int tilesx = (Wo + 127) / 128;
  const int tx = blockIdx.x % tilesx;
  int r = blockIdx.x / tilesx;
  const int tilesy = Hi;  // Ho / 8
  const int ty = r % tilesy;
  const int n = r / tilesy;
  const int ox = tx * 128 + (threadIdx.x & 31) * 4, oy = ty * 8 + (threadIdx.x >> 5);
  if (ox >= Wo) return;
  int iy1, ix1;
  float wy1, wy0, wx1[4], wx0[4];
  bilinear_taps<8>(oy, iy1, wy1, wy0);
#pragma unroll
  for (int j = 0; j < 4; ++j) bilinear_taps<8>(ox + j, ix1, wx1[j], wx0[j]);  // same ix1 for the 4 aligned pixels
  const __bf16* p00 = f + (((int64_t)n * (Hi + 2) + iy1) * (Wi + 2) + ix1) * U;
  const int64_t rowp = (int64_t)(Wi + 2) * U;
  float sc[4][CM];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < CM; ++k) sc[j][k] = 0.f;
  // software pipeline: the four 16-byte source loads of channel group g+1 are in flight while group g is
  // multiplied (few waves per SIMD fit beside 4*CM accumulators, so the loop must hide its own L2 latency)
  u32x4 n00 = *reinterpret_cast<const u32x4*>(p00), n01 = *reinterpret_cast<const u32x4*>(p00 + U);
  u32x4 n10 = *reinterpret_cast<const u32x4*>(p00 + rowp), n11 = *reinterpret_cast<const u32x4*>(p00 + rowp + U);
  for (int u0 = 0; u0 < U; u0 += 8) {
    const u32x4 a00 = n00, a01 = n01, a10 = n10, a11 = n11;
    const int un = u0 + 8 < U ? u0 + 8 : u0;
    n00 = *reinterpret_cast<const u32x4*>(p00 + un);
    n01 = *reinterpret_cast<const u32x4*>(p00 + U + un);
    n10 = *reinterpret_cast<const u32x4*>(p00 + rowp + un);
    n11 = *reinterpret_cast<const u32x4*>(p00 + rowp + U + un);
    const float* wrow = ws_g + u0 * C;
    if (u0 + 16 <= U)
      head_affine_group<CM, false>(a00, a01, a10, a11, wy0, wy1, wx0, wx1, wrow, sc_g + u0, sh_g + u0, C, 0, sc);
    else
      head_affine_group<CM, true>(a00, a01, a10, a11, wy0, wy1, wx0, wx1, wrow, sc_g + u0, sh_g + u0, C, (U - u0) * C, sc);
  }
  const int64_t opix = ((int64_t)n * Ho + oy) * Wo + ox;
  int64_t lab[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int k = 0; k < CM; ++k) sc[j][k] += bs_g[k < C ? k : C - 1];
    if (score) {
#pragma unroll
      for (int k = 0; k < CM; ++k)
        if (k < C) score[(opix + j) * C + k] = sc[j][k];
    }
    float m = sc[j][0];
#pragma unroll
    for (int k = 1; k < CM; ++k)
      if (k < C) m = fmaxf(m, sc[j][k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CM; ++k) {
      sc[j][k] = k < C ? xv_fast_exp(sc[j][k] - m) : 0.f;
      sum += sc[j][k];
    }
    const float rsum = xv_fast_rcp(sum);
    float best = -1.f;
    int bi = 0;
#pragma unroll
    for (int k = 0; k < CM; ++k) {
      const float p = sc[j][k] * rsum;
      if (k < C) {
        if (prob) prob[(opix + j) * C + k] = p;
        if (p > best) {
          best = p;
          bi = k;
        }
      }
    }
    lab[j] = bi;
  }
  if (label) {
    typedef __attribute__((ext_vector_type(2))) int64_t i64x2;
    *reinterpret_cast<i64x2*>(label + opix) = i64x2{lab[0], lab[1]};
    *reinterpret_cast<i64x2*>(label + opix + 2) = i64x2{lab[2], lab[3]};
  }
}

}  // namespace

// S = fused . Ws at 1/8 resolution into a zero-bordered fp32 [N][h+2][w+2][CM] buffer (shared by the
// forward head and the head backward)
extern "C" int xv_score_lowres(const xv_act* fused, const float* w_score, int num_classes, float* S, void* stream) {
  XV_REQUIRE_BF16(fused);
  XV_CHECK_ARG(fused && fused->data && w_score && S);
  XV_CHECK_SHAPE(fused->c > 0 && (fused->c & 7) == 0 && num_classes >= 1 && num_classes <= 32);
  const int64_t lowres = (int64_t)fused->n * (fused->h + 2) * (fused->w + 2);
  const unsigned g1 = (unsigned)((lowres + 127) / 128);
  hipStream_t s = (hipStream_t)stream;
  const __bf16* f = (const __bf16*)fused->data;
  XV_CHECK_SHAPE(fused->c <= 256);
#define XV_SL(CMV)                                                                                             \
  hipLaunchKernelGGL(score_lowres_kernel<CMV>, dim3(g1), dim3(128), (size_t)fused->c * CMV * 4, s, f, w_score, \
                     fused->n, fused->h, fused->w, fused->c, num_classes, S)
  XV_CM_SWITCH(num_classes, XV_SL)
#undef XV_SL
  return xv_launch_status();
}

// Fused head of a two-expert fusion model (see fused_head_kernel): Sa / Sb from xv_score_lowres of each expert's `fused`
// map; mode 0 = Bayes (tab = loglik [2][C][C], lognorm unused), 1 = Dirichlet (tab = am1 [2][C][C], lognorm [2][C]).
extern "C" int xv_fused_head_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi,
                                 int wi, int num_classes, int mode, const float* tab, const float* lognorm,
                                 const float* logprior, int64_t* fused_label, void* stream) {
  XV_CHECK_ARG(Sa && Sb && bias_a && bias_b && tab && logprior && fused_label && (mode == 0 || (mode == 1 && lognorm)));
  XV_CHECK_SHAPE(n > 0 && hi > 0 && wi > 0 && num_classes >= 1 && num_classes <= 32);
  // threads: four output pixels each (Bayes; Dirichlet in the packed form), one (Dirichlet, scalar form) -- see fused_head_kernel
  const int64_t nthreads = (int64_t)n * hi * 8 * wi * (mode == 0 ? 2 : 8);
  XV_CHECK_ARG(((uintptr_t)fused_label & 15) == 0);
  const unsigned grid = (unsigned)((nthreads + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  // XV_DIRICHLET_HEAD_PK=0: the scalar form of the Dirichlet head for C == CM too (read per call: the test that pins the two
  // forms to the same labels switches it)
  const char* pk_env = getenv("XV_DIRICHLET_HEAD_PK");
  const bool pk = !(pk_env && pk_env[0] == '0');
#define XV_FH(CMV)                                                                                                      \
  {                                                                                                                     \
    const size_t lds = (size_t)(2 * (mode == 0 ? num_classes : CMV) * CMV + 3 * CMV + (mode == 0 ? num_classes * num_classes : 0)) * 4; \
    if (mode == 0 && num_classes == CMV)                                                                                \
      hipLaunchKernelGGL((fused_head_kernel<CMV, 0, true>), dim3(grid), dim3(256), lds, s, Sa, Sb, bias_a, bias_b, n, hi, \
                         wi, num_classes, tab, lognorm, logprior, fused_label);                                         \
    else if (mode == 0)                                                                                                 \
      hipLaunchKernelGGL((fused_head_kernel<CMV, 0>), dim3(grid), dim3(256), lds, s, Sa, Sb, bias_a, bias_b, n, hi, wi,  \
                         num_classes, tab, lognorm, logprior, fused_label);                                             \
    else if (num_classes == CMV && pk && CMV <= 20) /* (the template argument below only keeps CMV > 20 from instantiating) */ \
      hipLaunchKernelGGL((fused_dirichlet_head_pk_kernel<(CMV <= 20 ? CMV : 4), 4>), dim3((grid + 3) / 4), dim3(256), lds, s, \
                         Sa, Sb, bias_a, bias_b, n, hi, wi, tab, lognorm, logprior, fused_label);                       \
    else if (num_classes == CMV)                                                                                        \
      hipLaunchKernelGGL((fused_head_kernel<CMV, 1, true>), dim3(grid), dim3(256), lds, s, Sa, Sb, bias_a, bias_b, n, hi, \
                         wi, num_classes, tab, lognorm, logprior, fused_label);                                         \
    else                                                                                                                \
      hipLaunchKernelGGL((fused_head_kernel<CMV, 1>), dim3(grid), dim3(256), lds, s, Sa, Sb, bias_a, bias_b, n, hi, wi,  \
                         num_classes, tab, lognorm, logprior, fused_label);                                             \
  }
  XV_CM_SWITCH(num_classes, XV_FH)
#undef XV_FH
  return xv_launch_status();
}

// Grid-scoring heads (see fused_head_grid_score_kernel / fused_head_joint_hist_kernel).  LDS of one launch: 40 KB, so that four
// 256-thread workgroups share a CU's 160 KB (the four waves per SIMD of the register budget); one grid point takes its tables
// and its [C][C] u32 counters.
static const size_t XV_GRID_SCORE_LDS = 40 * 1024;
static size_t grid_point_bytes(int num_classes) {
  const size_t cm = (size_t)(num_classes + 3) / 4 * 4;
  return (2 * cm * cm + 3 * cm + (size_t)num_classes * num_classes) * 4;
}

extern "C" int xv_fused_head_grid_capacity(int num_classes) {
  if (num_classes < 2 || num_classes > 32) return 0;
  return (int)(XV_GRID_SCORE_LDS / grid_point_bytes(num_classes));
}

// workgroups of a grid-stride launch over `items` (256 per workgroup and step): four per CU, or the caller's bound
static int grid_score_workgroups(int64_t items, int max_workgroups) {
  return xv_grid_for(items, 256, xv_grid_bound(4, 0, max_workgroups));
}

extern "C" int xv_fused_head_grid_score_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n,
                                            int hi, int wi, int num_classes, int num_points, const float* tab,
                                            const float* lognorm, const float* logprior, const int32_t* labels, int64_t* cm,
                                            int max_workgroups, void* stream) {
  XV_CHECK_ARG(Sa && Sb && bias_a && bias_b && tab && lognorm && logprior && labels && cm);
  XV_CHECK_ARG(num_classes >= 2 && num_points >= 1 && max_workgroups >= 0);
  XV_CHECK_SHAPE(num_classes <= 32 && xv_dims_sane(n, hi, wi));
  XV_CHECK_ARG(num_points <= xv_fused_head_grid_capacity(num_classes));
  const int64_t npix = (int64_t)n * hi * wi * 64;
  const int grid = grid_score_workgroups(npix, max_workgroups);
  XV_CHECK_SHAPE(npix / grid < ((int64_t)1 << 31));  // (a workgroup's u32 counters)
  const size_t lds = grid_point_bytes(num_classes) * num_points;
  hipStream_t s = (hipStream_t)stream;
#define XV_GS(CMV)                                                                                                          \
  hipLaunchKernelGGL(fused_head_grid_score_kernel<CMV>, dim3(grid), dim3(256), lds, s, Sa, Sb, bias_a, bias_b, n, hi, wi,    \
                     num_classes, num_points, tab, lognorm, logprior, labels, reinterpret_cast<unsigned long long*>(cm))
  XV_CM_SWITCH(num_classes, XV_GS)
#undef XV_GS
  return xv_launch_status();
}

extern "C" int xv_fused_head_joint_hist_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n,
                                            int hi, int wi, int num_classes, const int32_t* labels, int64_t* hist,
                                            int max_workgroups, void* stream) {
  XV_CHECK_ARG(Sa && Sb && bias_a && bias_b && labels && hist && ((uintptr_t)labels & 15) == 0);
  XV_CHECK_ARG(num_classes >= 2 && num_classes <= 20 && max_workgroups >= 0);  // 20^3 u32 counters: 32 KB of LDS
  XV_CHECK_SHAPE(xv_dims_sane(n, hi, wi));
  const int64_t nquads = (int64_t)n * hi * wi * 64 / xv_joint_hist_pixels((num_classes + 3) / 4 * 4);  // threads' pixel groups
  const int grid = grid_score_workgroups(nquads, max_workgroups);
  XV_CHECK_SHAPE(nquads / grid < ((int64_t)1 << 29));
  const size_t lds = (size_t)num_classes * num_classes * num_classes * 4;
  hipStream_t s = (hipStream_t)stream;
#define XV_JH(CMV)                                                                                                          \
  hipLaunchKernelGGL(fused_head_joint_hist_kernel<CMV>, dim3(grid), dim3(256), lds, s, Sa, Sb, bias_a, bias_b, n, hi, wi,    \
                     num_classes, labels, reinterpret_cast<unsigned long long*>(hist))
  XV_CM_SWITCH(num_classes, XV_JH)
#undef XV_JH
  return xv_launch_status();
}

// Fused average head (see fused_head_average_kernel), label and counting form.  A thread's pixel group (two pixels) must
// divide the output width 8 wi: it always does, the check stands for whoever changes the group.
#define XV_FA_LAUNCH(CMV, COUNT, GRID, LDS, FUSED, LABELS, CMP)                                                               \
  {                                                                                                                          \
    if (num_classes == CMV)                                                                                                  \
      hipLaunchKernelGGL((fused_head_average_kernel<CMV, COUNT, true>), dim3(GRID), dim3(256), LDS, s, Sa, Sb, bias_a, bias_b, \
                         n, hi, wi, num_classes, FUSED, LABELS, CMP);                                                        \
    else                                                                                                                     \
      hipLaunchKernelGGL((fused_head_average_kernel<CMV, COUNT, false>), dim3(GRID), dim3(256), LDS, s, Sa, Sb, bias_a,       \
                         bias_b, n, hi, wi, num_classes, FUSED, LABELS, CMP);                                                \
  }

extern "C" int xv_fused_head_average_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n,
                                         int hi, int wi, int num_classes, int64_t* fused_label, void* stream) {
  XV_CHECK_ARG(Sa && Sb && bias_a && bias_b && fused_label && ((uintptr_t)fused_label & 15) == 0);
  XV_CHECK_ARG(num_classes >= 1 && num_classes <= 32);
  XV_CHECK_SHAPE(xv_dims_sane(n, hi, wi));
  const int group = XV_AVERAGE_PIXELS;
  XV_CHECK_ARG(((int64_t)wi * 8) % group == 0);
  const int64_t nquads = (int64_t)n * hi * wi * 64 / group;
  XV_CHECK_SHAPE((nquads + 255) / 256 <= 0x7fffffff);
  const unsigned grid = (unsigned)((nquads + 255) / 256);
  const size_t lds = average_head_lds(num_classes, false);
  hipStream_t s = (hipStream_t)stream;
#define XV_FA(CMV) XV_FA_LAUNCH(CMV, false, grid, lds, fused_label, (const int32_t*)nullptr, (unsigned long long*)nullptr)
  XV_CM_SWITCH(num_classes, XV_FA)
#undef XV_FA
  return xv_launch_status();
}

extern "C" int xv_fused_head_average_count_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n,
                                               int hi, int wi, int num_classes, const int32_t* labels, int64_t* cm,
                                               int max_workgroups, void* stream) {
  XV_CHECK_ARG(Sa && Sb && bias_a && bias_b && labels && cm && ((uintptr_t)labels & 15) == 0);
  XV_CHECK_ARG(num_classes >= 1 && num_classes <= 32 && max_workgroups >= 0);
  XV_CHECK_SHAPE(xv_dims_sane(n, hi, wi));
  const int group = XV_AVERAGE_PIXELS;
  XV_CHECK_ARG(((int64_t)wi * 8) % group == 0);
  const int64_t nquads = (int64_t)n * hi * wi * 64 / group;
  const int grid = grid_score_workgroups(nquads, max_workgroups);
  XV_CHECK_SHAPE(nquads / grid < ((int64_t)1 << 29));  // (a workgroup's u32 counters)
  const size_t lds = average_head_lds(num_classes, true);
  hipStream_t s = (hipStream_t)stream;
#define XV_FA(CMV) \
  XV_FA_LAUNCH(CMV, true, grid, lds, (int64_t*)nullptr, labels, reinterpret_cast<unsigned long long*>(cm))
  XV_CM_SWITCH(num_classes, XV_FA)
#undef XV_FA
  return xv_launch_status();
}
#undef XV_FA_LAUNCH

// Fused head of a fusion model with two to four experts (see fused_head_multi_kernel): S[e] from xv_score_lowres of expert e's
// `fused` map.  mode 0 = Bayes (tab = loglik [E][C][C]), 1 = Dirichlet (tab = am1 [E][C][C], lognorm [E][C]), 2 = mean (no
// tables).  Everything is checked before anything is launched.
extern "C" int xv_fused_head_multi_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                                       int num_classes, int mode, const float* tab, const float* lognorm,
                                       const float* logprior, int64_t* fused_label, void* stream) {
  XV_CHECK_ARG(fused_label && ((uintptr_t)fused_label & 15) == 0 && xv_mode_tables_ok(mode, tab, lognorm, logprior));
  HeadPtrs ptrs;
  XV_CHECK_OK(xv_multi_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs));
  const int64_t nquads = (int64_t)n * hi * wi * 64 / xv_multi_pixels(mode);  // (8 wi is a multiple of every pixel group)
  XV_CHECK_SHAPE((nquads + 255) / 256 <= 0x7fffffff);
  const unsigned grid = (unsigned)((nquads + 255) / 256);
  const int ndec = mode == 0 ? multi_head_dec_entries(num_classes, num_experts) : 0;
  hipStream_t s = (hipStream_t)stream;
  // (this kernel keeps the lognorm slot [E][CM] in Bayes mode too, E CM floats more than xv_multi_table_floats; then dec)
  const size_t cm = ((size_t)num_classes + 3) / 4 * 4;
  const size_t lds = mode == 2 ? 0
                               : (num_experts * (mode == 1 ? cm : (size_t)num_classes) * cm + (num_experts + 1) * cm) * 4 +
                                     (size_t)(ndec + 15) / 16 * 16;
#define XV_FM_MODE(CMV, FULL, MODE)                                                                                        \
  hipLaunchKernelGGL((fused_head_multi_kernel<CMV, MODE, FULL>), dim3(grid), dim3(256), lds, s, ptrs, num_experts, n, hi, wi, \
                     num_classes, ndec, tab, lognorm, logprior, fused_label)
#define XV_FM(CMV)                                 \
  {                                                \
    if (num_classes == CMV)                        \
      XV_MODE_SWITCH(mode, XV_FM_MODE, CMV, true)  \
    else                                           \
      XV_MODE_SWITCH(mode, XV_FM_MODE, CMV, false) \
  }
  XV_CM_SWITCH(num_classes, XV_FM)
#undef XV_FM
#undef XV_FM_MODE
  return xv_launch_status();
}

// Variance head of the MC-dropout fusion model (see variance_head_kernel): Sa / Sb from xv_score_lowres of each expert's
// (T+1) n-image `fused` map, [(T+1) n][hi+2][wi+2][CP] each.
extern "C" int xv_variance_head_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi,
                                    int wi, int num_classes, int num_samples, int64_t* label, float* fused_score, float* probs,
                                    float* variance, void* stream) {
  XV_CHECK_ARG(Sa && Sb && bias_a && bias_b && label);
  XV_CHECK_SHAPE(num_classes >= 1 && num_classes <= 32 && num_samples >= 1 && num_samples <= 1024);
  XV_CHECK_SHAPE(xv_dims_sane(n, hi, wi) && (int64_t)n * (num_samples + 1) < ((int64_t)1 << 31));
  const int64_t npix = (int64_t)n * hi * wi * 64;
  XV_CHECK_SHAPE((npix + 255) / 256 <= 0x7fffffff);
  const unsigned grid = (unsigned)((npix + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
#define XV_VH(CMV)                                                                                                    \
  hipLaunchKernelGGL(variance_head_kernel<CMV>, dim3(grid), dim3(256), 0, s, Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, \
                     num_samples, label, fused_score, probs, variance)
  XV_CM_SWITCH(num_classes, XV_VH)
#undef XV_VH
  return xv_launch_status();
}

// Uncertainty head of the MC-dropout Bayesian FCN (see mc_uncertainty_head_kernel): S from xv_score_lowres of the T n-image
// `fused` map, [T n][hi+2][wi+2][CP], sample-major.
extern "C" int xv_mc_uncertainty_head_fwd(const float* S, const float* bias, int n, int hi, int wi, int num_classes,
                                          int num_samples, int64_t* label, float* mean_prob, float* entropy,
                                          float* cond_entropy, float* variance, void* stream) {
  XV_CHECK_ARG(S && bias && label && num_samples >= 1 && num_classes >= 2);
  XV_CHECK_SHAPE(num_classes <= 32 && num_samples <= 1024);
  XV_CHECK_SHAPE(xv_dims_sane(n, hi, wi) && (int64_t)n * num_samples < ((int64_t)1 << 31));
  const int64_t npix = (int64_t)n * hi * wi * 64;
  XV_CHECK_SHAPE((npix + 255) / 256 <= 0x7fffffff);
  const unsigned grid = (unsigned)((npix + 255) / 256);
  const float ln_c = xv_ln_classes(num_classes);
  hipStream_t s = (hipStream_t)stream;
#define XV_UH(CMV)                                                                                                          \
  hipLaunchKernelGGL(mc_uncertainty_head_kernel<CMV>, dim3(grid), dim3(256), 0, s, S, bias, n, hi, wi, num_classes, num_samples, \
                     ln_c, label, mean_prob, entropy, cond_entropy, variance)
  XV_CM_SWITCH(num_classes, XV_UH)
#undef XV_UH
  return xv_launch_status();
}

// Scoring form of the uncertainty head (see mc_uncertainty_score_kernel): S as xv_mc_uncertainty_head_fwd takes it.
extern "C" int xv_mc_uncertainty_score_fwd(const float* S, const float* bias, int n, int hi, int wi, int num_classes,
                                           int num_samples, float inv_temperature, const int32_t* labels, int mantissa_bits,
                                           int octaves, int fixed_row, uint64_t* hist, double* nll, int64_t* counts,
                                           void* stream) {
  XV_CHECK_ARG(S && bias && hist && num_samples >= 1 && num_classes >= 2 && inv_temperature > 0.f);
  XV_CHECK_ARG(mantissa_bits >= 3 && mantissa_bits <= 8 && octaves >= 8 && octaves <= 32);
  XV_CHECK_ARG(fixed_row >= -1 && fixed_row <= 1 && (fixed_row >= 0 || labels) && (!labels || (nll && counts)));
  XV_CHECK_SHAPE(num_classes <= 32 && num_samples <= 1024);
  XV_CHECK_SHAPE(xv_dims_sane(n, hi, wi) && (int64_t)n * num_samples < ((int64_t)1 << 31));
  const int64_t npix = (int64_t)n * hi * wi * 64;
  // one copy: three histograms of two rows and, with labels, the NLL sums and counts.  Copies while four workgroups fit a
  // CU's 160 KB of LDS (40 KB each); a single copy may take the 64 KB of the statistics kernels (two workgroups per CU).
  const size_t per_copy = (size_t)(octaves << mantissa_bits) * 6 * 4 + (labels ? (size_t)num_classes * 16 : 0);
  int rep = 8;
  while (rep > 1 && per_copy * rep > 40 * 1024) rep >>= 1;
  XV_CHECK_ARG(per_copy * rep <= 64 * 1024);
  const unsigned grid = (unsigned)xv_grid_for(npix, 256, xv_num_cus() * 4);
  const float ln_c = xv_ln_classes(num_classes);
  hipStream_t s = (hipStream_t)stream;
#define XV_US(CMV)                                                                                                          \
  hipLaunchKernelGGL(mc_uncertainty_score_kernel<CMV>, dim3(grid), dim3(256), per_copy * rep, s, S, bias, n, hi, wi, num_classes, \
                     num_samples, ln_c, inv_temperature, labels, mantissa_bits, octaves, fixed_row,                         \
                     reinterpret_cast<unsigned long long*>(hist), nll, reinterpret_cast<unsigned long long*>(counts), rep)
  XV_CM_SWITCH(num_classes, XV_US)
#undef XV_US
  return xv_launch_status();
}

// Moments pass of the uncertainty-weighted Dirichlet fusion (see uncertainty_moments_kernel): Sa / Sb as xv_variance_head_fwd
// takes them, [(T+1) n][hi+2][wi+2][CP] each.
extern "C" int xv_uncertainty_moments(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n, int hi,
                                      int wi, int num_classes, int num_samples, float* mvar, float* vmax, void* stream) {
  XV_CHECK_ARG(Sa && Sb && bias_a && bias_b && mvar && vmax && ((uintptr_t)vmax & 3) == 0);
  XV_CHECK_SHAPE(num_classes >= 1 && num_classes <= 32 && num_samples >= 1 && num_samples <= 1024);
  XV_CHECK_SHAPE(xv_dims_sane(n, hi, wi) && (int64_t)n * (num_samples + 1) < ((int64_t)1 << 31));
  const int64_t npix = (int64_t)n * hi * wi * 64;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(vmax, 0, 2 * sizeof(float), s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(xv_grid_for(npix, 512, 256), 2);
#define XV_UM(CMV)                                                                                                          \
  hipLaunchKernelGGL(uncertainty_moments_kernel<CMV>, grid, dim3(512), 0, s, Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, \
                     num_samples, mvar, reinterpret_cast<uint32_t*>(vmax))
  XV_CM_SWITCH(num_classes, XV_UM)
#undef XV_UM
  return xv_launch_status();
}

// Fusion head of the uncertainty-weighted Dirichlet fusion (see uncertainty_dirichlet_head_kernel): params float [2][C][C]
// with params[e][j][c] = A_e[j][c]; mvar / vmax from xv_uncertainty_moments.
extern "C" int xv_uncertainty_dirichlet_head_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b, int n,
                                                 int hi, int wi, int num_classes, const float* mvar, const float* vmax,
                                                 const float* params, const float* logprior, int64_t* label, float* fused_score,
                                                 float* probs, float* mix, void* stream) {
  XV_CHECK_ARG(Sa && Sb && bias_a && bias_b && mvar && vmax && params && logprior && label);
  XV_CHECK_SHAPE(num_classes >= 1 && num_classes <= 32 && xv_dims_sane(n, hi, wi));
  const int64_t npix = (int64_t)n * hi * wi * 64;
  XV_CHECK_SHAPE((npix + 255) / 256 <= 0x7fffffff);
  const unsigned grid = (unsigned)((npix + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
#define XV_UDH(CMV)                                                                                                         \
  hipLaunchKernelGGL(uncertainty_dirichlet_head_kernel<CMV>, dim3(grid), dim3(256),                                         \
                     (size_t)(2 * num_classes * CMV + 3 * CMV) * 4, s, Sa, Sb, bias_a, bias_b, n, hi, wi, num_classes, mvar, \
                     vmax, params, logprior, label, fused_score, probs, mix)
  XV_CM_SWITCH(num_classes, XV_UDH)
#undef XV_UDH
  return xv_launch_status();
}

extern "C" int xv_decoder_head_affine_fwd(const xv_act* fused, const float* scale, const float* shift,
                                         const float* w_score, const float* b_score, int num_classes, float* score,
                                         float* prob, int64_t* label, void* stream) {
  XV_REQUIRE_BF16(fused);
  XV_CHECK_ARG(fused && fused->data && scale && shift && w_score && b_score && (score || prob || label));
  XV_CHECK_ARG(!label || ((uintptr_t)label & 15) == 0);  // the kernel stores labels in 16-byte pairs
  XV_CHECK_SHAPE(fused->n > 0 && fused->h > 0 && fused->w > 0);
  XV_CHECK_SHAPE(fused->c > 0 && (fused->c & 7) == 0 && num_classes >= 1 && num_classes <= 32);
  const int Wo = fused->w * 8;
  const int64_t nblk = (int64_t)((Wo + 127) / 128) * fused->h * fused->n;
  XV_CHECK_SHAPE(nblk <= 0x7fffffff);
  hipStream_t s = (hipStream_t)stream;
  const __bf16* f = (const __bf16*)fused->data;
#define XV_HA(CMV)                                                                                                  \
  hipLaunchKernelGGL(decoder_head_affine_kernel<CMV>, dim3((unsigned)nblk), dim3(256), 0, s, f, scale, shift, w_score, \
                     b_score, fused->n, fused->h, fused->w, fused->c, num_classes, score, prob, label)
  XV_CM_SWITCH(num_classes, XV_HA)
#undef XV_HA
  return xv_launch_status();
}

extern "C" size_t xv_decoder_head_workspace_bytes(int n, int h, int w, int num_classes) {
  if (!xv_dims_sane(n, h, w) || num_classes < 1 || num_classes > 32) return 0;
  return (size_t)n * ((size_t)h + 2) * ((size_t)w + 2) * ((num_classes + 3) / 4 * 4) * sizeof(float);
}

// low-resolution class scores -> score / prob / label: the label alone (16-byte aligned) through the four-pixel form
static void launch_decoder_head(const float* S, const float* b_score, int n, int hi, int wi, int num_classes, float* score,
                                float* prob, int64_t* label, hipStream_t s) {
  const int64_t npix = (int64_t)n * hi * wi * 64;
  const bool label_only = !score && !prob && ((uintptr_t)label & 15) == 0;
  const unsigned g2 = (unsigned)(((label_only ? npix / 4 : npix) + 255) / 256);
#define XV_HEAD(CMV)                                                                                                     \
  {                                                                                                                      \
    if (label_only)                                                                                                      \
      hipLaunchKernelGGL(decoder_head_label4_kernel<CMV>, dim3(g2), dim3(256), 0, s, S, b_score, n, hi, wi, num_classes, \
                         label);                                                                                         \
    else                                                                                                                 \
      hipLaunchKernelGGL(decoder_head_kernel<CMV>, dim3(g2), dim3(256), 0, s, S, b_score, n, hi, wi, num_classes, score, \
                         prob, label);                                                                                   \
  }
  XV_CM_SWITCH(num_classes, XV_HEAD)
#undef XV_HEAD
}

extern "C" int xv_decoder_head_fwd(const xv_act* fused, const float* w_score, const float* b_score, int num_classes,
                                   float* score, float* prob, int64_t* label, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  XV_REQUIRE_BF16(fused);
  XV_CHECK_ARG(fused && fused->data && w_score && b_score && workspace);
  XV_CHECK_ARG(score || prob || label);
  XV_CHECK_SHAPE(fused->n > 0 && fused->h > 0 && fused->w > 0);
  XV_CHECK_SHAPE(fused->c > 0 && (fused->c & 7) == 0 && num_classes >= 1 && num_classes <= 32);
  if (workspace_bytes < xv_decoder_head_workspace_bytes(fused->n, fused->h, fused->w, num_classes)) return XV_EWORKSPACE;
  XV_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
  hipStream_t s = (hipStream_t)stream;
  float* S = (float*)workspace;
  const int64_t npix = (int64_t)fused->n * fused->h * fused->w * 64;
  XV_CHECK_SHAPE((npix + 255) / 256 <= 0x7fffffff);
  {
    const int rc = xv_score_lowres(fused, w_score, num_classes, S, stream);
    if (rc != XV_OK) return rc;
  }
  launch_decoder_head(S, b_score, fused->n, fused->h, fused->w, num_classes, score, prob, label, s);
  return xv_launch_status();
}

// The second half of xv_decoder_head_fwd alone: low-resolution class scores S (float32 [N][hi+2][wi+2][CP], zero border;
// from xv_score_lowres or xv_score_lowres_f32) -> score / prob / label at 8x the resolution.
extern "C" int xv_decoder_head_from_scores(const float* S, const float* b_score, int n, int hi, int wi, int num_classes,
                                           float* score, float* prob, int64_t* label, void* stream) {
  XV_CHECK_ARG(S && b_score && (score || prob || label));
  XV_CHECK_SHAPE(n > 0 && hi > 0 && wi > 0 && num_classes >= 1 && num_classes <= 32);
  const int64_t npix = (int64_t)n * hi * wi * 64;
  XV_CHECK_SHAPE((npix + 255) / 256 <= 0x7fffffff);
  launch_decoder_head(S, b_score, n, hi, wi, num_classes, score, prob, label, (hipStream_t)stream);
  return xv_launch_status();
}

extern "C" int xv_softmax_argmax(const float* score, int64_t npix, int num_classes, float* prob, int64_t* label,
                                 void* stream) {
  XV_CHECK_ARG(score && (prob || label));
  XV_CHECK_SHAPE(npix > 0 && num_classes >= 1 && num_classes <= 32);
  hipStream_t s = (hipStream_t)stream;
  const bool al16 = (((uintptr_t)score | (uintptr_t)prob) & 15) == 0;  // (the vector form of a 12-class map: xv_softmax_argmax
  //                                                                         takes any float pointer)
  if (num_classes == 12 && al16)
    hipLaunchKernelGGL(softmax_argmax_kernel<12>, dim3(xv_grid_for(npix)), dim3(256), 0, s, score, npix, num_classes, prob,
                       label);
  else if (num_classes <= 16)
    hipLaunchKernelGGL(softmax_argmax_kernel<16>, dim3(xv_grid_for(npix)), dim3(256), 0, s, score, npix, num_classes, prob,
                       label);
  else
    hipLaunchKernelGGL(softmax_argmax_kernel<32>, dim3(xv_grid_for(npix)), dim3(256), 0, s, score, npix, num_classes, prob,
                       label);
  return xv_launch_status();
}
