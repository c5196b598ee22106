// Calibration scoring of one pixel, written ONCE for the kernel on materialised maps and the fused head (calibration.hip):
// equal class scores give equal bins, equal fixed-point confidences and equal NLL terms by construction.
//
// For class scores s[k], k < C, in the log domain, the winner `win` (the first maximum, decided by the caller: a temperature
// never moves it), a temperature T > 0 and the ground truth `label`:
//   z    = sum_k exp((s[k] - s[win]) / T)            ascending k, an IEEE division per class, xv_fast_exp (v_exp_f32)
//   conf = 1.0f / z                                   an IEEE division
//   q    = (uint32)(conf 2^24)                        truncation; 0 <= q <= 2^24 whatever the scores hold (NaN gives 0)
//   bin  = min(q >> (24 - bin_bits), NB - 1)          NB = 1 << bin_bits
//   nll  = min(ln z - (s[label] - s[win]) / T, -ln 1e-10)      xv_fast_log; the clip of xv_unc_nll_term
// Contraction is off inside: no caller's context decides where an fma forms.
#pragma once

#include "xv_common.h"

constexpr int XV_CALIB_MAXT = 16;             // temperatures of one launch, at most (they travel as a kernel argument)
constexpr int XV_CALIB_NLL_COPIES = 32;       // copies of every NLL sum in LDS, copy = lane & 31
constexpr float XV_CALIB_NLL_CLIP = 23.025850929940457f;  // -ln 1e-10

struct CalibTemps {
  float t[XV_CALIB_MAXT];
};

// a probability into the log domain: the mean fusion's class score, and a materialised probability map's (kind 1)
__device__ static __forceinline__ float calib_log_prob(float p) {
#pragma clang fp contract(off)
  return xv_fast_log(1e-20f + p);
}

// first maximum of v[k], k < C: the decision of fuse_argmax_prior (xv_fuse.h) on scores that already hold the prior
template <int CM>
__device__ static __forceinline__ int calib_first_max(const float (&v)[CM], int C) {
  float best = 0.f;
  int bi = 0;
#pragma unroll
  for (int k = 0; k < CM; ++k)
    if (k < C && (k == 0 || v[k] > best)) {
      best = v[k];
      bi = k;
    }
  return bi;
}

// s[idx] with a run-time index on statically indexed registers: a chain of selects.  The empty asm (no instruction) keeps the
// optimizer from folding the chain back into an indexed load, which would put the whole array into scratch memory.
template <int CM>
__device__ static __forceinline__ float calib_pick(const float (&s)[CM], int idx) {
  float v = s[0];
#pragma unroll
  for (int k = 1; k < CM; ++k) {
    v = k == idx ? s[k] : v;
    asm volatile("" : "+v"(v));
  }
  return v;
}

// One class's term of z and its exponent d = (s[k] - s[win]) / T; calib_conf: the confidence of a finished z.  The two
// statements calib_pixel and conf_pixel (xv_conf.h) share: a confidence map's q IS the q counted here.
__device__ static __forceinline__ float calib_term(float s_k, float s_win, float T, float& d) {
#pragma clang fp contract(off)
  d = (s_k - s_win) / T;
  return xv_fast_exp(d);
}

__device__ static __forceinline__ float calib_conf(float z) {
#pragma clang fp contract(off)
  return 1.0f / z;
}

// the fixed-point confidence: truncation, 0 <= q <= 2^24 whatever conf holds (NaN gives 0)
__device__ static __forceinline__ uint32_t calib_q(float conf) {
#pragma clang fp contract(off)
  return (uint32_t)fminf(fmaxf(conf * 16777216.f, 0.f), 16777216.f);
}

// One pixel at one temperature: s_win = s[win], s_lab = s[label] (calib_pick, taken once per pixel by the caller; s_lab is
// ignored by a caller that drops nll).  Lanes k >= C are ignored.
template <int CM>
__device__ static __forceinline__ void calib_pixel(const float (&s)[CM], int C, float s_win, float s_lab, float T, int bin_bits,
                                                   uint32_t& q, int& bin, float& nll) {
#pragma clang fp contract(off)
  float z = 0.f;
#pragma unroll
  for (int k = 0; k < CM; ++k)
    if (k < C) {
      float d;
      z = z + calib_term(s[k], s_win, T, d);
    }
  q = calib_q(calib_conf(z));
  const int top = (1 << bin_bits) - 1;
  const int b = (int)(q >> (24 - bin_bits));
  bin = b < top ? b : top;
  nll = fminf(xv_fast_log(z) - (s_lab - s_win) / T, XV_CALIB_NLL_CLIP);
}

// One wave's pixels of one table and temperature -> its LDS cells.  A cell is two 64-bit words: count in the low and correct
// in the high half of the first (a workgroup counts fewer than 2^31 pixels per image, so the halves never carry), the sum of q
// in the second -- 257 pixels at confidence 1 pass 32 bits, so that column is 64 bits WIDE in LDS, not split; a pixel costs two
// ds_add_u64.  THE TOP BIN: trained experts put most pixels there, all 64 lanes of a wave on one address.  Its lanes are
// aggregated first -- a ballot counts them and the correct ones, their q (at most 64 x 2^24 = 2^30, so 32 bits hold the wave's
// sum) is summed by six xor shuffles, one lane adds the two words -- whenever two or more lanes hold it; every
// other bin is added lane by lane (at ten bin bits two lanes of a wave rarely share one).  The NLL term goes to copy lane & 31
// of its double sum: two lanes per address.  `bin` < 0: nothing to count.  Every lane of the wave calls it, converged.
__device__ static __forceinline__ void calib_wave_add(unsigned long long* cells, double* nll_s, int bin, int top, bool correct,
                                                      uint32_t q, float nll) {
  const int lane = (int)__lane_id();
  const bool in_top = bin == top;
  const unsigned long long tops = __ballot(in_top);
  bool single = bin >= 0;
  if (__popcll(tops) >= 2) {  // (wave-uniform)
    uint32_t qs = in_top ? q : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) qs += (uint32_t)__shfl_xor((int)qs, off, 64);
    const unsigned long long right = __ballot(in_top && correct);
    if (lane == __builtin_ctzll(tops)) {
      atomicAdd(&cells[2 * top], (unsigned long long)__popcll(tops) | ((unsigned long long)__popcll(right) << 32));
      atomicAdd(&cells[2 * top + 1], (unsigned long long)qs);
    }
    single = single && !in_top;
  }
  if (single) {
    atomicAdd(&cells[2 * bin], 1ull | ((unsigned long long)(correct ? 1 : 0) << 32));
    atomicAdd(&cells[2 * bin + 1], (unsigned long long)q);
  }
  if (bin >= 0) atomicAdd(&nll_s[lane & (XV_CALIB_NLL_COPIES - 1)], (double)nll);
}
