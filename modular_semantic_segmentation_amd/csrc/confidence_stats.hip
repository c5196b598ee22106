// Uncertainty benchmarks of a posterior for gfx950: the three confidence values of confidence.hip -- entropy, 1 - conf,
// 1 - margin -- binned by row (misclassified or not; in- or out-of-distribution) instead of written, with the NLL sums and
// class counts of the valid pixels: the tables uncertainty_model.py turns into ROC curves, without a per-pixel map.
//
// THE COUNT of a pixel is conf_stats_pixel (xv_conf_stats.h), the ONE place it is written; its arithmetic is conf_pixel's
// (xv_conf.h) and, for the NLL term, calib_pixel's (xv_calib.h).
//
//   xv_confidence_stats                         from a materialised map of scores or probabilities
//   xv_fused_head_multi_confidence_stats_fwd    from the experts' low-resolution scores: the statements of
//                                               fused_head_multi_confidence_kernel (confidence.hip) up to the fused scores
//                                               and `win`, then the count; on request every expert's own tables from its
//                                               interpolated logits, as fused_head_multi_calibration_kernel takes them
//
// LDS.  Per table (the fusion's, then one per expert) the replicated block of xv_common.h: hist u32 [3][2][bins][rep], and
// with labels nll double [C][rep] and counts u64 [C][rep]; one copy of one table may take 64 KB (the rule of
// xv_uncertainty_stats), all tables of a launch with the staged fusion tables 160 KB.  Copies (rep, a power of two, at most
// 8) are added while two workgroups fit a CU's 160 KB.  The NLL terms are float, added as doubles into the copies, the copies
// summed per workgroup, one double atomic per class and workgroup: the sums of calibration.hip.
//
// GRID.  512-thread workgroups (two waves per SIMD each, as the calibration kernels), two per CU and never above 512
// (docs/HISTORY.md: kernels that end in atomics on few addresses), pixels in a grid-stride loop, so a workgroup zeroes, stages
// and flushes ONCE: one 64-bit global atomic per non-zero cell.  A workgroup's share of the pixels stays below 2^32 (checked).
#include "xv_common.h"
#include "xv_heads.h"  // the heads' per-pixel pieces and, through it, xv_fuse.h (sets `fp contract(on)` for what follows)
#include "xv_conf_stats.h"
#include "xv_multi.h"  // the host side: argument checks and the grid bound

namespace {

constexpr int XV_CS_THREADS = 512;
constexpr int XV_CS_PER_CU = 2;
constexpr int XV_CS_MAX_GRID = 512;
constexpr int XV_CS_LDS = 160 * 1024;     // one workgroup's LDS on gfx950
constexpr int XV_CS_ONE_COPY = 64 * 1024;  // one copy of one table, at most

// where a launch adds its tables: the fusion's (or the only one), then the experts' [E][...] (null: none)
struct ConfStatsOut {
  unsigned long long* hist;
  double* nll;
  unsigned long long* counts;
  unsigned long long* expert_hist;
  double* expert_nll;
  unsigned long long* expert_counts;
};

// table t of a workgroup's LDS: the NLL blocks of all tables come first (doubles), then the histograms
__device__ static __forceinline__ ConfStatsTable conf_stats_table(double* nll_s, uint32_t* hist_s, int t, const ConfStatsHow& how) {
  return ConfStatsTable{nll_s + (int64_t)t * 2 * how.ncls * how.rep, hist_s + (int64_t)t * 6 * (how.octaves << how.M) * how.rep};
}

// every table of the workgroup into the global ones; every thread of the workgroup calls it after a barrier
__device__ static __forceinline__ void conf_stats_flush(double* nll_s, uint32_t* hist_s, int ntables, int C, const ConfStatsHow& how,
                                                        const ConfStatsOut& out) {
  const int cells = 6 * (how.octaves << how.M);
  for (int t = 0; t < ntables; ++t) {
    const ConfStatsTable tbl = conf_stats_table(nll_s, hist_s, t, how);
    if (t == 0)
      xv_unc_tables_flush(tbl.nll, how.ncls, tbl.hist, cells, how.rep, out.hist, out.nll, out.counts);
    else
      xv_unc_tables_flush(tbl.nll, how.ncls, tbl.hist, cells, how.rep, out.expert_hist + (int64_t)(t - 1) * cells,
                          out.expert_nll + (int64_t)(t - 1) * C, out.expert_counts + (int64_t)(t - 1) * C);
  }
}

// waves per SIMD the Dirichlet forms are held to, as confidence.hip holds its own (xv_conf_waves): left alone the compiler
// keeps table rows of the rolled expert loop in registers.  One class step below that file's thresholds: with the experts'
// counting beside the fusion, 20 classes at four waves and 28 at three spill (36 and 76 bytes of scratch).
constexpr int xv_cs_waves(int cm, int mode) { return mode != 1 ? 2 : (cm <= 16 ? 4 : (cm <= 24 ? 3 : 2)); }

// ---- from the experts' low-resolution scores: the statements of fused_head_multi_confidence_kernel up to v and win --------
template <int CM, int MODE>
__global__ __launch_bounds__(XV_CS_THREADS) __attribute__((amdgpu_waves_per_eu(xv_cs_waves(CM, MODE)))) void
fused_head_multi_confidence_stats_kernel(HeadPtrs ptrs, int E, int N, int Hi, int Wi, int C, const float* __restrict__ tab_g,
                                         const float* __restrict__ lognorm_g, const float* __restrict__ logprior_g,
                                         const int32_t* __restrict__ labels, ConfStatsHow how, int ntables, ConfStatsOut out) {
  extern __shared__ __attribute__((aligned(16))) float cs_tab[];
  const int rows = MODE == 1 ? CM : C;  // table rows per expert
  const int ntab = MODE == 2 ? 0 : E * rows * CM + (MODE == 1 ? E * CM : 0) + CM;
  float* ln = cs_tab + E * rows * CM;            // [E][CM], Dirichlet only
  float* lp = ln + (MODE == 1 ? E * CM : 0);     // [CM]
  double* nll_s = reinterpret_cast<double*>(cs_tab + (ntab + 3) / 4 * 4);
  uint32_t* hist_s = reinterpret_cast<uint32_t*>(nll_s + (int64_t)ntables * 2 * how.ncls * how.rep);
  if (threadIdx.x < 256) {  // (the staging helpers stride by 256)
    if constexpr (MODE == 0) fuse_stage_rows<CM>(cs_tab, tab_g, E * C, C);
    if constexpr (MODE == 1) fuse_stage_dirichlet<CM>(cs_tab, ln, tab_g, lognorm_g, E, C);
    if constexpr (MODE != 2) fuse_stage_rows<CM>(lp, logprior_g, 1, C);
  }
  xv_unc_tables_zero(nll_s, ntables * how.ncls, hist_s, ntables * 6 * (how.octaves << how.M), how.rep);
  __syncthreads();
  const bool experts = ntables > 1;
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t ppi = (int64_t)Ho * Wo;  // pixels of one image
  const int64_t total = (int64_t)N * ppi;
  for (int64_t at = (int64_t)blockIdx.x * XV_CS_THREADS + threadIdx.x; at < total; at += (int64_t)gridDim.x * XV_CS_THREADS) {
    const int img = (int)(at / ppi);
    const int64_t pix = at - (int64_t)img * ppi;
    const int ox = (int)(pix % Wo);
    const int oy = (int)(pix / Wo);
    int iy1, ix1;
    float wy1, wy0, wx1, wx0;
    bilinear_taps<8>(oy, iy1, wy1, wy0);
    bilinear_taps<8>(ox, ix1, wx1, wx0);
    const int l = labels != nullptr ? labels[at] : -1;
    // running state over the experts: Bayes their labels in one word, 5 bits each, l_0 first; Dirichlet and mean the sum
    constexpr int NTOT = MODE == 0 ? 1 : CM;
    float total_s[NTOT];
    (void)total_s;
    int key = 0;
#pragma nounroll
    for (int e = 0; e < E; ++e) {
      const float* S = head_ptr(ptrs.s, e);
      const float* bs = head_ptr(ptrs.b, e);
      f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
      head_load_taps<CM>(S, img, iy1, ix1, Hi, Wi, ta, tb, tc, td);
      float sc[CM];
      head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, bs, C, sc);
      // the expert's own tables from its logits, before the softmax overwrites them
      if (experts) conf_stats_pixel<CM>(sc, C, calib_first_max<CM>(sc, C), l, how, conf_stats_table(nll_s, hist_s, 1 + e, how));
      const float m = head_max<CM>(sc, C);
      if constexpr (MODE == 0) {
        int le = head_label_fast<CM>(sc, m, C);
        if (le < 0) le = head_softmax<CM>(sc, m, C);
        key = key * 32 + le;
      } else if constexpr (MODE == 2) {
        head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
#pragma unroll
        for (int k = 0; k < CM; ++k) total_s[k] = e == 0 ? sc[k] : total_s[k] + sc[k];
      } else {
        head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
        fuse_renorm_log<CM, true>(sc, C);
        // the fmaf chain over k of dirichlet_fuse_kernel per class, two classes per v_pk_fma_f32 on the transposed table
        // (padded classes / terms are exact zeros: fma(0, 0, d) = d), as fused_head_multi_kernel
        f32x2 dot2[CM / 2];
#pragma unroll
        for (int cp = 0; cp < CM / 2; ++cp) dot2[cp] = f32x2{0.f, 0.f};
#pragma unroll
        for (int k = 0; k < CM; ++k) {
          const f32x2* rowk = reinterpret_cast<const f32x2*>(cs_tab + (e * CM + k) * CM);
          const f32x2 lk = f32x2{sc[k], sc[k]};
#pragma unroll
          for (int cp = 0; cp < CM / 2; ++cp) dot2[cp] = __builtin_elementwise_fma(rowk[cp], lk, dot2[cp]);
        }
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          const float L = dot2[c >> 1][c & 1] - ln[e * CM + c];
          total_s[c] = c < C ? (e == 0 ? L : total_s[c] + L) : 0.f;
        }
      }
    }
    // the fused class scores in the log domain and their first maximum
    float v[CM];
    int win;
    if constexpr (MODE == 0) {
      // bayes_fuse_kernel: the E rows of the pixel's labels summed in ascending expert order, then the prior
      float sc[CM];
#pragma nounroll
      for (int e = 0; e < E; ++e) {
        const int le = (key >> (5 * (E - 1 - e))) & 31;
        const f32x4* row = reinterpret_cast<const f32x4*>(cs_tab + (e * C + le) * CM);
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
      for (int k = 0; k < CM; ++k) v[k] = sc[k] + lp[k];
      win = calib_first_max<CM>(v, C);
    } else if constexpr (MODE == 1) {
#pragma unroll
      for (int k = 0; k < CM; ++k) v[k] = total_s[k] + lp[k];
      win = calib_first_max<CM>(v, C);
    } else {
      // average_fuse_kernel: total / E by an IEEE division, its first maximum; then the log domain
      const float fe = (float)E;
#pragma unroll
      for (int k = 0; k < CM; ++k) v[k] = total_s[k] / fe;
      win = calib_first_max<CM>(v, C);
#pragma unroll
      for (int k = 0; k < CM; ++k) v[k] = calib_log_prob(v[k]);
    }
    conf_stats_pixel<CM>(v, C, win, l, how, conf_stats_table(nll_s, hist_s, 0, how));
  }
  __syncthreads();
  conf_stats_flush(nll_s, hist_s, ntables, C, how, out);
}

// ---- from a materialised map: values float [npix][C], scores (kind 0) or probabilities (kind 1) ---------------------------
template <int CM>
__global__ __launch_bounds__(XV_CS_THREADS) void confidence_stats_kernel(const float* __restrict__ values, int kind, int64_t npix,
                                                                         int C, int vec, const int32_t* __restrict__ labels,
                                                                         ConfStatsHow how, ConfStatsOut out) {
  extern __shared__ __attribute__((aligned(16))) float cs_tab[];
  double* nll_s = reinterpret_cast<double*>(cs_tab);
  uint32_t* hist_s = reinterpret_cast<uint32_t*>(nll_s + (int64_t)2 * how.ncls * how.rep);
  xv_unc_tables_zero(nll_s, how.ncls, hist_s, 6 * (how.octaves << how.M), how.rep);
  __syncthreads();
  const ConfStatsTable tbl = conf_stats_table(nll_s, hist_s, 0, how);
  for (int64_t at = (int64_t)blockIdx.x * XV_CS_THREADS + threadIdx.x; at < npix; at += (int64_t)gridDim.x * XV_CS_THREADS) {
    const float* row = values + at * C;
    float v[CM];
    if (vec) {  // (C is a multiple of four and the map 16-byte aligned)
#pragma unroll
      for (int k4 = 0; k4 < CM / 4; ++k4) {
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (4 * k4 < C) r = *reinterpret_cast<const f32x4*>(row + 4 * k4);
        v[4 * k4] = r.x, v[4 * k4 + 1] = r.y, v[4 * k4 + 2] = r.z, v[4 * k4 + 3] = r.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < CM; ++k) v[k] = k < C ? row[k] : 0.f;
    }
    const int win = calib_first_max<CM>(v, C);
    if (kind == 1) {
#pragma unroll
      for (int k = 0; k < CM; ++k) v[k] = calib_log_prob(v[k]);
    }
    conf_stats_pixel<CM>(v, C, win, labels != nullptr ? labels[at] : -1, how, tbl);
  }
  __syncthreads();
  conf_stats_flush(nll_s, hist_s, 1, C, how, out);
}

// The temperature, the bins, the row rule and the fusion's three tables -> how (without rep) and out.  hist is required; nll
// and counts with labels; labels unless the row is fixed; every pointer aligned to its element.
bool conf_stats_args_ok(float temperature, const int32_t* labels, int mantissa_bits, int octaves, int fixed_row, int num_classes,
                        uint64_t* hist, double* nll, int64_t* counts, ConfStatsHow& how, ConfStatsOut& out) {
  if (!(temperature > 0.f) || !(temperature <= 3.4028234663852886e38f)) return false;  // (NaN fails the first test)
  if (mantissa_bits < 3 || mantissa_bits > 8 || octaves < 8 || octaves > 32) return false;
  if (fixed_row < -1 || fixed_row > 1 || (fixed_row < 0 && labels == nullptr)) return false;
  if (hist == nullptr || (labels != nullptr && (nll == nullptr || counts == nullptr))) return false;
  if (((uintptr_t)labels & 3) != 0 || (((uintptr_t)hist | (uintptr_t)nll | (uintptr_t)counts) & 7) != 0) return false;
  how = ConfStatsHow{temperature, mantissa_bits, octaves, fixed_row, labels != nullptr ? num_classes : 0, 1};
  out = ConfStatsOut{reinterpret_cast<unsigned long long*>(hist), nll, reinterpret_cast<unsigned long long*>(counts),
                     nullptr, nullptr, nullptr};
  return true;
}

// bytes of one copy of one table
size_t conf_stats_table_bytes(const ConfStatsHow& how) {
  return (size_t)(how.octaves << how.M) * 6 * 4 + (size_t)how.ncls * 16;
}

// copies of the tables: doubled while two workgroups fit a CU's LDS beside `fixed` bytes of fusion tables, at most 8
int conf_stats_copies(size_t one_copy, size_t fixed) {
  int rep = 1;
  while (rep < 8 && fixed + one_copy * rep * 2 <= (size_t)XV_CS_LDS / XV_CS_PER_CU) rep <<= 1;
  return rep;
}

// the bounded grid; XV_ESHAPE where a workgroup's share of the pixels could pass a 32-bit counter
int conf_stats_grid(int64_t npix, int& grid) {
  const int64_t need = (npix + XV_CS_THREADS - 1) / XV_CS_THREADS;
  const int bound = xv_grid_bound(XV_CS_PER_CU, XV_CS_MAX_GRID, 0);
  grid = (int)(need < bound ? need : bound);
  XV_CHECK_SHAPE((need + grid - 1) / grid * XV_CS_THREADS < ((int64_t)1 << 32));
  return XV_OK;
}

}  // namespace

extern "C" int xv_confidence_stats(const float* values, int kind, int n, int64_t ppi, int num_classes, float temperature,
                                   const int32_t* labels, int mantissa_bits, int octaves, int fixed_row, uint64_t* hist,
                                   double* nll, int64_t* counts, void* stream) {
  XV_CHECK_ARG(values && ((uintptr_t)values & 3) == 0 && n >= 1 && ppi >= 1 && (kind == 0 || kind == 1));
  XV_CHECK_ARG(num_classes >= 2 && num_classes <= 32);
  ConfStatsHow how;
  ConfStatsOut out;
  XV_CHECK_ARG(conf_stats_args_ok(temperature, labels, mantissa_bits, octaves, fixed_row, num_classes, hist, nll, counts, how, out));
  const size_t one = conf_stats_table_bytes(how);
  XV_CHECK_ARG(one <= (size_t)XV_CS_ONE_COPY);
  XV_CHECK_SHAPE(ppi <= ((int64_t)1 << 40) / n);
  const int64_t npix = (int64_t)n * ppi;
  int grid;
  XV_CHECK_OK(conf_stats_grid(npix, grid));
  how.rep = conf_stats_copies(one, 0);
  const size_t lds = one * how.rep;
  const int vec = (num_classes & 3) == 0 && ((uintptr_t)values & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
#define XV_CS(CMV)                                                                                                           \
  {                                                                                                                          \
    static bool attr[XV_MAX_DEVICES] = {false};                                                                              \
    const hipError_t e = xv_allow_dynamic_lds(reinterpret_cast<const void*>(&confidence_stats_kernel<CMV>), XV_CS_LDS, attr, \
                                              false);                                                                        \
    if (e != hipSuccess) return (int)e;                                                                                      \
    hipLaunchKernelGGL(confidence_stats_kernel<CMV>, dim3(grid), dim3(XV_CS_THREADS), lds, s, values, kind, npix,            \
                       num_classes, vec, labels, how, out);                                                                  \
  }
  XV_CM_SWITCH(num_classes, XV_CS)
#undef XV_CS
  return xv_launch_status();
}

extern "C" int xv_fused_head_multi_confidence_stats_fwd(const float* const* S, const float* const* bias, int num_experts, int n,
                                                        int hi, int wi, int num_classes, int mode, const float* tab,
                                                        const float* lognorm, const float* logprior, float temperature,
                                                        const int32_t* labels, int mantissa_bits, int octaves, int fixed_row,
                                                        uint64_t* hist, double* nll, int64_t* counts, uint64_t* expert_hist,
                                                        double* expert_nll, int64_t* expert_counts, void* stream) {
  XV_CHECK_ARG(xv_mode_tables_ok(mode, tab, lognorm, logprior));
  XV_CHECK_ARG(xv_experts_classes_ok(num_experts, num_classes));  // (before the tables are sized for 1 + num_experts)
  ConfStatsHow how;
  ConfStatsOut out;
  XV_CHECK_ARG(conf_stats_args_ok(temperature, labels, mantissa_bits, octaves, fixed_row, num_classes, hist, nll, counts, how, out));
  // the experts' tables: all three or none (without labels their NLL sums and counts stay untouched, as the fusion's)
  const bool experts = expert_hist != nullptr;
  XV_CHECK_ARG((expert_nll != nullptr) == experts && (expert_counts != nullptr) == experts);
  XV_CHECK_ARG((((uintptr_t)expert_hist | (uintptr_t)expert_nll | (uintptr_t)expert_counts) & 7) == 0);
  out.expert_hist = reinterpret_cast<unsigned long long*>(expert_hist);
  out.expert_nll = expert_nll;
  out.expert_counts = reinterpret_cast<unsigned long long*>(expert_counts);
  const int ntables = experts ? 1 + num_experts : 1;
  const size_t one = conf_stats_table_bytes(how) * ntables;
  const size_t fixed = (xv_multi_table_floats(mode, num_experts, num_classes) + 3) / 4 * 16;
  XV_CHECK_ARG(conf_stats_table_bytes(how) <= (size_t)XV_CS_ONE_COPY && fixed + one <= (size_t)XV_CS_LDS);
  HeadPtrs ptrs;
  XV_CHECK_OK(xv_multi_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs));
  int grid;
  XV_CHECK_OK(conf_stats_grid((int64_t)n * hi * wi * 64, grid));
  how.rep = conf_stats_copies(one, fixed);
  const size_t lds = fixed + one * how.rep;
  hipStream_t s = (hipStream_t)stream;
#define XV_CF_MODE(CMV, MODE)                                                                                                \
  {                                                                                                                          \
    static bool attr[XV_MAX_DEVICES] = {false};                                                                              \
    const hipError_t err = xv_allow_dynamic_lds(                                                                             \
        reinterpret_cast<const void*>(&fused_head_multi_confidence_stats_kernel<CMV, MODE>), XV_CS_LDS, attr, false);        \
    if (err != hipSuccess) return (int)err;                                                                                  \
    hipLaunchKernelGGL((fused_head_multi_confidence_stats_kernel<CMV, MODE>), dim3(grid), dim3(XV_CS_THREADS), lds, s, ptrs, \
                       num_experts, n, hi, wi, num_classes, tab, lognorm, logprior, labels, how, ntables, out);              \
  }
#define XV_CF(CMV) XV_MODE_SWITCH(mode, XV_CF_MODE, CMV)
  XV_CM_SWITCH(num_classes, XV_CF)
#undef XV_CF
#undef XV_CF_MODE
  return xv_launch_status();
}
