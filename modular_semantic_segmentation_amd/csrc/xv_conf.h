// The confidence of one pixel, written ONCE for the kernel on materialised maps and the fused head (confidence.hip).
//
// For class scores s[k], k < C, in the log domain, the winner `win` (the first maximum, decided by the caller: a temperature
// never moves it) and a temperature T > 0, with calib_term / calib_conf of xv_calib.h -- the statements calib_pixel counts by,
// so that (uint32)(conf 2^24) of a written confidence is exactly the q of the reliability tables:
//   d_k     = (s[k] - s[win]) / T                       an IEEE division per class
//   e_k     = xv_fast_exp(d_k)
//   z       = sum_k e_k                                 ascending k
//   conf    = 1.0f / z
//   entropy = max(0, ln z - (sum_k e_k d_k) / z)        nats, xv_fast_log; a term with e_k == 0 adds nothing (no 0 * inf)
//   margin  = conf - (max_{k != win} e_k) / z           in [0, 1]; exactly 0 where the maximum is tied (e_k = e_win = 1)
// Contraction is off inside: no caller's context decides where an fma forms.
#pragma once

#include "xv_calib.h"

// s_win = s[win] (calib_pick, taken by the caller).  Lanes k >= C are ignored.
template <int CM>
__device__ static __forceinline__ void conf_pixel(const float (&s)[CM], int C, int win, float s_win, float T, float& conf,
                                                  float& entropy, float& margin) {
#pragma clang fp contract(off)
  float z = 0.f, ed = 0.f, second = 0.f;
#pragma unroll
  for (int k = 0; k < CM; ++k)
    if (k < C) {
      float d;
      const float e = calib_term(s[k], s_win, T, d);
      z = z + e;
      if (e != 0.f) ed = ed + e * d;
      if (k != win) second = fmaxf(second, e);
    }
  conf = calib_conf(z);
  entropy = fmaxf(xv_fast_log(z) - ed / z, 0.f);
  margin = fminf(fmaxf(conf - second / z, 0.f), 1.f);
}

// the label a confidence map writes: void below the threshold (a threshold of 0 voids nothing: conf < 0 never holds)
__device__ static __forceinline__ int64_t conf_label(int win, float conf, float threshold, int64_t void_label) {
  return conf < threshold ? void_label : (int64_t)win;
}
