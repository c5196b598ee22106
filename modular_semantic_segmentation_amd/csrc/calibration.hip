// Calibration scoring for gfx950: can the confidence of a posterior be believed?  The reliability table of the fused posterior
// (and of every expert's own), from which the host takes ECE, MCE, over-confidence and the NLL, at several temperatures at once.
//
// THE TABLE.  Class scores s[k], k < C, in the log domain: the fused score xv_bayes_fuse / xv_dirichlet_fuse write to
// score_out; for the mean ln(1e-20 + mean_e p_e[k]); for one expert its logits.  `win` is the first maximum -- the label the
// existing route writes; a temperature never moves it -- and per temperature T > 0 (xv_calib.h: calib_pixel, the ONE place the
// arithmetic is written)
//   z = sum_k exp((s[k] - s[win]) / T), conf = 1 / z, q = (uint32)(conf 2^24), bin = min(q >> (24 - bin_bits), NB - 1),
//   correct = (win == label), nll = min(ln z - (s[label] - s[win]) / T, -ln 1e-10)
// and over the pixels with 0 <= label < C
//   table[group][t][bin] += (1, correct, q)       int64 [num_groups][num_temperatures][NB][3]
//   nll[group][t]        += nll                   double [num_groups][num_temperatures]
// both accumulated, not cleared.  Count, correct and the fixed-point confidence sum are integers: groups, ranks and repeated
// launches add exactly.  For probabilities (the mean fusion, kind 1) `win` is the first maximum of the PROBABILITIES, the
// decision of xv_average_fuse; the logarithm is monotone, so it is a maximum of s too.
//
//   xv_calibration_table                  from a materialised map of scores or probabilities
//   xv_fused_head_multi_calibration_fwd   from the experts' low-resolution scores: fused_head_multi_agreement_kernel
//                                         (agreement.hip) with this table counted in place of the agreement cell, and on
//                                         request every expert's own table from its interpolated logits
//   xv_calibration_capacity               temperatures one launch serves
//
// LDS.  A cell is 16 bytes -- count and correct packed in one 64-bit word, the q sum 64 bits wide (257 pixels at confidence 1
// pass 32 bits; not split) -- so a table of one temperature is 16 NB bytes (16 KB at ten bin bits) plus 32 double copies of its
// NLL sum (256 bytes).  Of a workgroup's 160 KB, 20 KB are kept for the fusion tables of the fused form (17 KB at 32 classes,
// four experts, Dirichlet) and the temperatures; capacity = min(16, 140 KB / (num_tables (16 NB + 256))): 8 temperatures for the
// fusion alone at ten bin bits, 1 with four experts' tables beside it.  A launch asks for what it uses, not for 160 KB.
// THE TOP BIN is aggregated per wave before the LDS atomic (xv_calib.h: calib_wave_add says how).
//
// Work is dealt out in (image, part) slots (xv_multi.h: xv_slot_plan); a flush costs one 64-bit global atomic per non-zero
// column of a non-empty bin; the trip count is uniform over the workgroup; the grid is bounded, two 512-thread workgroups per
// CU and at most 512.  group == nullptr: every image is group 0.  A group id is checked before anything is indexed with it.
#include "xv_common.h"
#include "xv_heads.h"  // the heads' per-pixel pieces and, through it, xv_fuse.h (sets `fp contract(on)` for what follows)
#include "xv_calib.h"
#include "xv_multi.h"  // the host side: argument checks and the slot plan

namespace {

constexpr int XV_CALIB_THREADS = 512;
constexpr int XV_CALIB_MAX_GRID = 512;
constexpr int XV_CALIB_LDS = 160 * 1024;      // one workgroup's LDS on gfx950
constexpr int XV_CALIB_RESERVE = 20 * 1024;   // the fusion tables of the fused form and the temperatures

int calib_capacity(int bin_bits, int num_tables) {
  if (bin_bits < 4 || bin_bits > 10 || num_tables < 1 || num_tables > 1 + XV_MULTI_MAXE) return 0;
  const int per = num_tables * ((16 << bin_bits) + XV_CALIB_NLL_COPIES * 8);
  const int cap = (XV_CALIB_LDS - XV_CALIB_RESERVE) / per;
  return cap < XV_CALIB_MAXT ? cap : XV_CALIB_MAXT;
}

// the temperatures from the kernel argument into LDS (static indices: the argument never becomes a private copy)
__device__ static __forceinline__ void calib_stage_temps(float* tl, const CalibTemps& temps) {
#pragma unroll
  for (int i = 0; i < XV_CALIB_MAXT; ++i)
    if (threadIdx.x == i) tl[i] = temps.t[i];
}

// one workgroup's cells of one image into the global tables; every thread of the workgroup calls it between two barriers.
// LDS table 0 is the fusion's (or the only one), table 1 + e expert e's.
__device__ static __forceinline__ void calib_flush(const unsigned long long* cells, const double* nll_s, int ntables, int NT,
                                                   int NB, int grp, unsigned long long* __restrict__ table,
                                                   double* __restrict__ nll, unsigned long long* __restrict__ expert_table,
                                                   double* __restrict__ expert_nll) {
  const int per = NT * NB, E = ntables - 1;
  for (int i = threadIdx.x; i < ntables * per; i += blockDim.x) {
    const unsigned long long cc = cells[2 * i];
    if (cc == 0ull) continue;
    const int tbl = i / per, r = i - tbl * per;
    unsigned long long* dst = tbl == 0 ? table + ((int64_t)grp * per + r) * 3
                                       : expert_table + (((int64_t)grp * E + (tbl - 1)) * per + r) * 3;
    const unsigned long long right = cc >> 32, qs = cells[2 * i + 1];
    atomicAdd(&dst[0], cc & 0xffffffffull);
    if (right) atomicAdd(&dst[1], right);
    if (qs) atomicAdd(&dst[2], qs);
  }
  for (int i = threadIdx.x; i < ntables * NT; i += blockDim.x) {
    double s = 0.0;
    for (int r = 0; r < XV_CALIB_NLL_COPIES; ++r) s += nll_s[i * XV_CALIB_NLL_COPIES + r];
    if (s != 0.0) {
      const int tbl = i / NT, t = i - tbl * NT;
      atomicAdd(tbl == 0 ? &nll[(int64_t)grp * NT + t] : &expert_nll[((int64_t)grp * E + (tbl - 1)) * NT + t], s);
    }
  }
}

// one pixel's scores -> the cells of LDS table `tbl` at every temperature
template <int CM>
__device__ static __forceinline__ void calib_count(const float (&s)[CM], int C, int win, int l, bool valid, const float* tl, int NT,
                                                   int bin_bits, int tbl, unsigned long long* cells, double* nll_s) {
  const int NB = 1 << bin_bits;
  const float s_win = calib_pick<CM>(s, win), s_lab = calib_pick<CM>(s, valid ? l : 0);
#pragma nounroll
  for (int t = 0; t < NT; ++t) {
    uint32_t q;
    int bin;
    float nl;
    calib_pixel<CM>(s, C, s_win, s_lab, tl[t], bin_bits, q, bin, nl);
    calib_wave_add(cells + (int64_t)(tbl * NT + t) * NB * 2, nll_s + (tbl * NT + t) * XV_CALIB_NLL_COPIES, valid ? bin : -1,
                   NB - 1, win == l, q, nl);
  }
}

// ---- from the experts' low-resolution scores: the statements of fused_head_multi_agreement_kernel up to the fused scores --
template <int CM, int MODE>
__global__ __launch_bounds__(XV_CALIB_THREADS) void fused_head_multi_calibration_kernel(
    HeadPtrs ptrs, int E, int N, int Hi, int Wi, int C, const float* __restrict__ tab_g, const float* __restrict__ lognorm_g,
    const float* __restrict__ logprior_g, const int32_t* __restrict__ labels, const int32_t* __restrict__ group, int NG,
    int parts, CalibTemps temps, int NT, int bin_bits, int ntables, unsigned long long* __restrict__ table,
    double* __restrict__ nll, unsigned long long* __restrict__ expert_table, double* __restrict__ expert_nll) {
  extern __shared__ __attribute__((aligned(16))) float cal_tab[];
  const int rows = MODE == 1 ? CM : C;  // table rows per expert
  const int ntab = MODE == 2 ? 0 : E * rows * CM + (MODE == 1 ? E * CM : 0) + CM;
  float* ln = cal_tab + E * rows * CM;            // [E][CM], Dirichlet only
  float* lp = ln + (MODE == 1 ? E * CM : 0);      // [CM]
  float* tl = cal_tab + ntab;                     // [XV_CALIB_MAXT]
  const int NB = 1 << bin_bits;
  const int ncells = ntables * NT * NB;
  unsigned long long* cells = reinterpret_cast<unsigned long long*>(cal_tab + (ntab + XV_CALIB_MAXT + 3) / 4 * 4);
  double* nll_s = reinterpret_cast<double*>(cells + 2 * (int64_t)ncells);  // [ntables][NT][copies]
  if (threadIdx.x < 256) {  // (the staging helpers stride by 256)
    if constexpr (MODE == 0) fuse_stage_rows<CM>(cal_tab, tab_g, E * C, C);
    if constexpr (MODE == 1) fuse_stage_dirichlet<CM>(cal_tab, ln, tab_g, lognorm_g, E, C);
    if constexpr (MODE != 2) fuse_stage_rows<CM>(lp, logprior_g, 1, C);
  }
  calib_stage_temps(tl, temps);
  const bool experts = ntables > 1;
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t ppi = (int64_t)Ho * Wo;  // pixels of one image
  const int64_t slots = (int64_t)N * parts;
  for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const int img = (int)(slot / parts), part = (int)(slot - (int64_t)img * parts);
    const int grp = group != nullptr ? group[img] : 0;
    if (grp < 0 || grp >= NG) continue;  // (uniform over the workgroup)
    for (int i = threadIdx.x; i < 2 * ncells; i += XV_CALIB_THREADS) cells[i] = 0ull;
    for (int i = threadIdx.x; i < ntables * NT * XV_CALIB_NLL_COPIES; i += XV_CALIB_THREADS) nll_s[i] = 0.0;
    __syncthreads();  // (the first one also publishes the tables and the temperatures)
    for (int64_t base = (int64_t)part * XV_CALIB_THREADS; base < ppi; base += (int64_t)parts * XV_CALIB_THREADS) {
      const bool live = base + threadIdx.x < ppi;
      if (__ballot(live) == 0) continue;  // (wave-uniform)
      const int64_t pix = live ? base + threadIdx.x : ppi - 1;
      const int ox = (int)(pix % Wo);
      const int oy = (int)(pix / Wo);
      int iy1, ix1;
      float wy1, wy0, wx1, wx0;
      bilinear_taps<8>(oy, iy1, wy1, wy0);
      bilinear_taps<8>(ox, ix1, wx1, wx0);
      const int l = live ? labels[(int64_t)img * ppi + pix] : -1;
      const bool valid = l >= 0 && l < C;
      // running state over the experts: Bayes their labels in one word, 5 bits each, l_0 first; Dirichlet and mean the sum
      constexpr int NTOT = MODE == 0 ? 1 : CM;
      float total[NTOT];
      (void)total;
      int key = 0;
#pragma nounroll
      for (int e = 0; e < E; ++e) {
        const float* S = head_ptr(ptrs.s, e);
        const float* bs = head_ptr(ptrs.b, e);
        f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
        head_load_taps<CM>(S, img, iy1, ix1, Hi, Wi, ta, tb, tc, td);
        float sc[CM];
        head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, bs, C, sc);
        // the expert's own table from its logits, before the softmax overwrites them
        if (experts) calib_count<CM>(sc, C, calib_first_max<CM>(sc, C), l, valid, tl, NT, bin_bits, 1 + e, cells, nll_s);
        const float m = head_max<CM>(sc, C);
        if constexpr (MODE == 0) {
          int le = head_label_fast<CM>(sc, m, C);
          if (le < 0) le = head_softmax<CM>(sc, m, C);
          key = key * 32 + le;
        } else if constexpr (MODE == 2) {
          head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
#pragma unroll
          for (int k = 0; k < CM; ++k) total[k] = e == 0 ? sc[k] : total[k] + sc[k];
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
            const f32x2* rowk = reinterpret_cast<const f32x2*>(cal_tab + (e * CM + k) * CM);
            const f32x2 lk = f32x2{sc[k], sc[k]};
#pragma unroll
            for (int cp = 0; cp < CM / 2; ++cp) dot2[cp] = __builtin_elementwise_fma(rowk[cp], lk, dot2[cp]);
          }
#pragma unroll
          for (int c = 0; c < CM; ++c) {
            const float L = dot2[c >> 1][c & 1] - ln[e * CM + c];
            total[c] = c < C ? (e == 0 ? L : total[c] + L) : 0.f;
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
          const f32x4* row = reinterpret_cast<const f32x4*>(cal_tab + (e * C + le) * CM);
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
        for (int k = 0; k < CM; ++k) v[k] = total[k] + lp[k];
        win = calib_first_max<CM>(v, C);
      } else {
        // average_fuse_kernel: total / E by an IEEE division, its first maximum; then the log domain
        const float fe = (float)E;
#pragma unroll
        for (int k = 0; k < CM; ++k) v[k] = total[k] / fe;
        win = calib_first_max<CM>(v, C);
#pragma unroll
        for (int k = 0; k < CM; ++k) v[k] = calib_log_prob(v[k]);
      }
      calib_count<CM>(v, C, win, l, valid, tl, NT, bin_bits, 0, cells, nll_s);
    }
    __syncthreads();
    calib_flush(cells, nll_s, ntables, NT, NB, grp, table, nll, expert_table, expert_nll);
    __syncthreads();  // (the next slot clears the cells)
  }
}

// ---- from a materialised map: values float [n][ppi][C], scores (KIND 0) or probabilities (KIND 1) -------------------------
template <int CM>
__global__ __launch_bounds__(XV_CALIB_THREADS) void calibration_table_kernel(
    const float* __restrict__ values, int kind, const int32_t* __restrict__ labels, const int32_t* __restrict__ group, int N,
    int64_t ppi, int C, int NG, int parts, CalibTemps temps, int NT, int bin_bits, int vec,
    unsigned long long* __restrict__ table, double* __restrict__ nll) {
  extern __shared__ __attribute__((aligned(16))) float cal_tab[];
  float* tl = cal_tab;  // [XV_CALIB_MAXT]
  const int NB = 1 << bin_bits;
  const int ncells = NT * NB;
  unsigned long long* cells = reinterpret_cast<unsigned long long*>(cal_tab + XV_CALIB_MAXT);
  double* nll_s = reinterpret_cast<double*>(cells + 2 * (int64_t)ncells);  // [NT][copies]
  calib_stage_temps(tl, temps);
  const int64_t slots = (int64_t)N * parts;
  for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const int img = (int)(slot / parts), part = (int)(slot - (int64_t)img * parts);
    const int grp = group != nullptr ? group[img] : 0;
    if (grp < 0 || grp >= NG) continue;  // (uniform over the workgroup)
    for (int i = threadIdx.x; i < 2 * ncells; i += XV_CALIB_THREADS) cells[i] = 0ull;
    for (int i = threadIdx.x; i < NT * XV_CALIB_NLL_COPIES; i += XV_CALIB_THREADS) nll_s[i] = 0.0;
    __syncthreads();  // (the first one also publishes the temperatures)
    for (int64_t base = (int64_t)part * XV_CALIB_THREADS; base < ppi; base += (int64_t)parts * XV_CALIB_THREADS) {
      const bool live = base + threadIdx.x < ppi;
      if (__ballot(live) == 0) continue;  // (wave-uniform)
      const int64_t at = (int64_t)img * ppi + (live ? base + threadIdx.x : ppi - 1);
      const int l = live ? labels[at] : -1;
      const bool valid = l >= 0 && l < C;
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
      calib_count<CM>(v, C, win, l, valid, tl, NT, bin_bits, 0, cells, nll_s);
    }
    __syncthreads();
    calib_flush(cells, nll_s, 1, NT, NB, grp, table, nll, table, nll);  // (one table: the expert pointers are never used)
    __syncthreads();  // (the next slot clears the cells)
  }
}

// bin bits, temperature count (against the capacity for `num_tables`) and every temperature finite and positive
bool calib_args_ok(const float* temperatures, int num_temperatures, int bin_bits, int num_tables, CalibTemps& temps) {
  const int cap = calib_capacity(bin_bits, num_tables);
  if (cap < 1 || temperatures == nullptr || num_temperatures < 1 || num_temperatures > cap) return false;
  for (int i = 0; i < XV_CALIB_MAXT; ++i) {
    const float t = temperatures[i < num_temperatures ? i : 0];
    if (!(t > 0.f) || !(t <= 3.4028234663852886e38f)) return false;  // (NaN fails the first test)
    temps.t[i] = t;
  }
  return true;
}

// the slot plan of both forms: two 512-thread workgroups per CU, never above 512, or the caller's bound; the 32-bit counters
// are a cell's count and correct halves
int calib_plan(int64_t ppi, int n, int max_workgroups, XvSlotPlan& plan) {
  return xv_slot_plan(ppi, XV_CALIB_THREADS, ppi, n, xv_grid_bound(2, XV_CALIB_MAX_GRID, max_workgroups), plan);
}

}  // namespace

extern "C" int xv_calibration_capacity(int bin_bits, int num_tables) { return calib_capacity(bin_bits, num_tables); }

extern "C" int xv_calibration_table(const float* values, int kind, const int32_t* labels, const int32_t* group, int n,
                                    int64_t ppi, int num_classes, const float* temperatures, int num_temperatures, int bin_bits,
                                    int num_groups, int64_t* table, double* nll, void* stream) {
  XV_CHECK_ARG(values && labels && table && nll && n >= 1 && ppi >= 1 && (kind == 0 || kind == 1));
  XV_CHECK_ARG(((uintptr_t)values & 3) == 0 && ((uintptr_t)labels & 3) == 0 && xv_group_ok(group, num_groups));
  XV_CHECK_ARG(((uintptr_t)table & 7) == 0 && ((uintptr_t)nll & 7) == 0);
  XV_CHECK_ARG(num_classes >= 2 && num_classes <= 32);
  CalibTemps temps;
  XV_CHECK_ARG(calib_args_ok(temperatures, num_temperatures, bin_bits, 1, temps));
  XV_CHECK_SHAPE(ppi <= ((int64_t)1 << 40) / n);
  XvSlotPlan plan;
  XV_CHECK_OK(calib_plan(ppi, n, 0, plan));
  const size_t lds = XV_CALIB_MAXT * 4 + (size_t)num_temperatures * ((16u << bin_bits) + XV_CALIB_NLL_COPIES * 8);
  const int vec = (num_classes & 3) == 0 && ((uintptr_t)values & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
#define XV_CT(CMV)                                                                                                          \
  {                                                                                                                         \
    static bool attr[XV_MAX_DEVICES] = {false};                                                                             \
    const hipError_t e =                                                                                                    \
        xv_allow_dynamic_lds(reinterpret_cast<const void*>(&calibration_table_kernel<CMV>), XV_CALIB_LDS, attr, false);     \
    if (e != hipSuccess) return (int)e;                                                                                     \
    hipLaunchKernelGGL(calibration_table_kernel<CMV>, dim3(plan.grid), dim3(XV_CALIB_THREADS), lds, s, values, kind, labels, \
                       group, n, ppi, num_classes, num_groups, plan.parts, temps, num_temperatures, bin_bits, vec,          \
                       reinterpret_cast<unsigned long long*>(table), nll);                                                  \
  }
  XV_CM_SWITCH(num_classes, XV_CT)
#undef XV_CT
  return xv_launch_status();
}

extern "C" int xv_fused_head_multi_calibration_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi,
                                                   int wi, int num_classes, int mode, const float* tab, const float* lognorm,
                                                   const float* logprior, const int32_t* labels, const int32_t* group,
                                                   int num_groups, const float* temperatures, int num_temperatures, int bin_bits,
                                                   int64_t* table, double* nll, int64_t* expert_table, double* expert_nll,
                                                   int max_workgroups, void* stream) {
  XV_CHECK_ARG(labels && table && nll && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)table & 7) == 0 && ((uintptr_t)nll & 7) == 0);
  XV_CHECK_ARG((expert_table == nullptr) == (expert_nll == nullptr));
  XV_CHECK_ARG(((uintptr_t)expert_table & 7) == 0 && ((uintptr_t)expert_nll & 7) == 0);
  XV_CHECK_ARG(xv_mode_tables_ok(mode, tab, lognorm, logprior) && xv_group_ok(group, num_groups) && max_workgroups >= 0);
  XV_CHECK_ARG(xv_experts_classes_ok(num_experts, num_classes));  // (before the capacity is asked for 1 + num_experts tables)
  const int ntables = expert_table != nullptr ? 1 + num_experts : 1;
  CalibTemps temps;
  XV_CHECK_ARG(calib_args_ok(temperatures, num_temperatures, bin_bits, ntables, temps));
  HeadPtrs ptrs;
  XV_CHECK_OK(xv_multi_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs));
  XvSlotPlan plan;
  XV_CHECK_OK(calib_plan((int64_t)hi * wi * 64, n, max_workgroups, plan));  // (one image's pixels)
  const size_t lds = (xv_multi_table_floats(mode, num_experts, num_classes) + XV_CALIB_MAXT + 3) / 4 * 16 +
                     (size_t)ntables * num_temperatures * ((16u << bin_bits) + XV_CALIB_NLL_COPIES * 8);
  hipStream_t s = (hipStream_t)stream;
#define XV_CF_MODE(CMV, MODE)                                                                                               \
  {                                                                                                                         \
    static bool attr[XV_MAX_DEVICES] = {false};                                                                             \
    const hipError_t err = xv_allow_dynamic_lds(                                                                            \
        reinterpret_cast<const void*>(&fused_head_multi_calibration_kernel<CMV, MODE>), XV_CALIB_LDS, attr, false);         \
    if (err != hipSuccess) return (int)err;                                                                                 \
    hipLaunchKernelGGL((fused_head_multi_calibration_kernel<CMV, MODE>), dim3(plan.grid), dim3(XV_CALIB_THREADS), lds, s,   \
                       ptrs, num_experts, n, hi, wi, num_classes, tab, lognorm, logprior, labels, group, num_groups,        \
                       plan.parts, temps, num_temperatures, bin_bits, ntables, reinterpret_cast<unsigned long long*>(table), \
                       nll, reinterpret_cast<unsigned long long*>(expert_table), expert_nll);                               \
  }
#define XV_CF(CMV) XV_MODE_SWITCH(mode, XV_CF_MODE, CMV)
  XV_CM_SWITCH(num_classes, XV_CF)
#undef XV_CF
#undef XV_CF_MODE
  return xv_launch_status();
}
