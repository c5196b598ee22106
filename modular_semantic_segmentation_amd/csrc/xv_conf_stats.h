// The uncertainty benchmarks' count of one pixel's confidence values, written ONCE for the kernel on materialised maps and the
// fused head (confidence_stats.hip): what confidence.hip writes per pixel, binned by row instead.
//
// For class scores s[k], k < C, in the log domain, their first maximum `win` and a temperature T > 0, conf_pixel (xv_conf.h)
// gives conf, entropy and margin; the three metrics, larger = less certain, each ONE IEEE operation from a written map value:
//   entropy            the entropy conf_pixel returns
//   least_confidence   1.0f - conf
//   small_margin       1.0f - margin
// and hist[metric][row][xv_unc_bin(value)] += 1 with row = (win != label) over the pixels with 0 <= label < C, or the
// caller's fixed row over every pixel.  With labels, over the valid pixels, nll[label] += nll_pixel -- calib_pixel's
// (xv_calib.h: min(ln z - (s[label] - s[win]) / T, -ln 1e-10), on the z conf_pixel sums) -- and counts[label] += 1.
//
// LDS.  One table is the replicated block of xv_common.h (xv_unc_tables_zero / xv_unc_tables_flush): nll double [ncls][rep],
// cnt u64 [ncls][rep], hist u32 [3][2][bins][rep], copy = lane & (rep - 1) fastest.  Confidence maps are spatially smooth and
// trained experts put whole waves into bin 0 of least_confidence, so the lanes that share the FIRST active lane's cell are
// counted by a ballot and added by that lane alone; every other lane adds its own 1.
#pragma once

#include "xv_conf.h"

// one table's block in a workgroup's LDS
struct ConfStatsTable {
  double* nll;     // [ncls][rep], then cnt u64 [ncls][rep]
  uint32_t* hist;  // [3][2][bins][rep]
};

// how a launch counts: the temperature, the bins, the row rule, and the shape of the LDS blocks
struct ConfStatsHow {
  float temperature;
  int M, octaves, fixed_row;
  int ncls;  // C with labels, 0 without: no NLL tables
  int rep;
};

// hist[cell] += 1 for every active lane: the lanes on the first active lane's cell in one add
__device__ static __forceinline__ void conf_stats_add(uint32_t* hist, int cell, int rep) {
  const int lane = (int)__lane_id();
  const int first = __builtin_amdgcn_readfirstlane(cell);
  const unsigned long long same = __ballot(cell == first);
  uint32_t* dst = &hist[cell * rep + (lane & (rep - 1))];
  if (cell != first)
    atomicAdd(dst, 1u);
  else if (lane == __builtin_ctzll(same))
    atomicAdd(dst, (uint32_t)__popcll(same));
}

// One pixel's scores and winner -> the cells of one LDS table.  l is the pixel's label (-1 without labels).
template <int CM>
__device__ static __forceinline__ void conf_stats_pixel(const float (&s)[CM], int C, int win, int l, const ConfStatsHow& how,
                                                        const ConfStatsTable& tbl) {
#pragma clang fp contract(off)
  const float s_win = calib_pick<CM>(s, win);
  float conf, entropy, margin;
  conf_pixel<CM>(s, C, win, s_win, how.temperature, conf, entropy, margin);
  const bool valid = l >= 0 && l < C;
  const int bins = how.octaves << how.M;
  if (how.fixed_row >= 0 || valid) {
    const int row = how.fixed_row >= 0 ? how.fixed_row : (win != l);
    conf_stats_add(tbl.hist, row * bins + xv_unc_bin(entropy, how.M, how.octaves), how.rep);
    conf_stats_add(tbl.hist, (2 + row) * bins + xv_unc_bin(1.0f - conf, how.M, how.octaves), how.rep);
    conf_stats_add(tbl.hist, (4 + row) * bins + xv_unc_bin(1.0f - margin, how.M, how.octaves), how.rep);
  }
  if (how.ncls != 0 && valid) {
    uint32_t q;
    int bin;
    float nl;
    calib_pixel<CM>(s, C, s_win, calib_pick<CM>(s, l), how.temperature, 10, q, bin, nl);
    const int copy = l * how.rep + ((int)__lane_id() & (how.rep - 1));
    atomicAdd(&tbl.nll[copy], (double)nl);
    atomicAdd(reinterpret_cast<unsigned long long*>(tbl.nll + how.ncls * how.rep) + copy, 1ull);
  }
}
