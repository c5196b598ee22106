// Expert-agreement tables for gfx950: what the confusion matrices of the counting heads (marginals, one per method) cannot
// say -- on how many pixels the experts disagree, whom the fusion follows there, what it loses and what it rescues.
//
// THE TABLE.  E experts (2..4), C classes; for every pixel with 0 <= label < C
//   mask       bit e is set iff expert e's label equals the ground truth                                  (0 .. 2^E - 1)
//   unanimous  1 iff all E experts give the same label, else 0
//   outcome    0 = the fused label equals the ground truth
//              1 = the fused label is wrong and equals at least one expert's label
//              2 = the fused label is wrong and equals no expert's label
//   table[group][label][mask][unanimous][outcome] += 1,   int64 [num_groups][C][2^E][2][3], accumulated, not cleared.
// Cells that cannot occur stay zero: unanimous = 1 with a mask other than 0 or 2^E - 1, and mask = 2^E - 1 with unanimous = 0.
// mask = 2^E - 1 does NOT fix the outcome (a Dirichlet fusion may leave unanimous, correct experts); nothing is special-cased.
//
//   xv_fused_head_multi_agreement_fwd   from the experts' low-resolution scores: fused_head_multi_kernel (heads.hip) with the
//                                       table counted in place of the label map; no label or probability map is written
//   xv_agreement_table                  from materialised label maps: the route for everything the fused heads do not serve
//
// The fused form, per output pixel and expert, ascending expert order, the statements of fused_head_multi_kernel at one pixel
// per thread: head_load_taps / head_eval_taps / head_max, then
//   MODE 0, Bayes      head_label_fast, head_softmax when it returns -1; after the experts the rows of the pixel's labels summed
//                      ((tab_0[l_0][k] + tab_1[l_1][k]) + ...), fuse_argmax_prior                       (bayes_fuse_kernel's order)
//   MODE 1, Dirichlet  head_softmax, fuse_renorm_log, the ascending-k fma chains on the transposed table (two classes per
//                      v_pk_fma_f32), - lognorm, total = L_0, += L_1, ..., fuse_argmax_prior        (dirichlet_fuse_kernel's order)
//   MODE 2, mean       head_softmax, s = ((p_0 + p_1) + ...), fuse_argmax_mean                       (average_fuse_kernel's order)
// so the fused label is the one xv_fused_head_multi_fwd writes and l_e the one decoder_head_kernel stores, bit for bit.  The
// staging, the renormalise-and-log and the decisions are xv_fuse.h's; the Bayes row sum and the Dirichlet chains are written
// out, as in every head (xv_fuse.h says why they are not functions).  The experts run in a rolled loop on running state in
// EVERY mode -- the labels packed into one word (5 bits each, l_0 first) and, Dirichlet and mean, total [CM]: with one
// parameter set nothing of size E x CM is kept, so unlike fused_head_multi_count_kernel there is one instantiation per class
// step and mode, whatever the expert count, and it carries strictly less state than that kernel does.
//
// ONE xv_wave_count per pixel (the counting head: E + 1).  Counters are u32 in LDS, C 2^E 6 of them: 12 KB at 32 classes and
// four experts, 2.3 KB at 12 classes and three.  With the tables (Bayes [E][C][CM] + [CM]; Dirichlet [E][CM][CM] + [E][CM] +
// [CM]: 16.6 KB at most) a workgroup holds under 29 KB, so the LDS never limits the residency the grid asks for.
//
// Work is dealt out in (image, part) slots (xv_multi.h: xv_slot_plan); the trip count is uniform over the workgroup
// (xv_wave_count needs whole waves; a lane past the end recomputes the image's last pixel and counts nothing).  The grid is
// bounded, at most 512 workgroups: two 512-thread workgroups per CU, the resident waves of the counting head's four of 256.
// group == nullptr: every image is group 0.  A group id is checked before anything is indexed with it.
#include "xv_common.h"
#include "xv_heads.h"  // the heads' per-pixel pieces and, through it, xv_fuse.h (sets `fp contract(on)` for what follows)
#include "xv_multi.h"  // the host side: argument checks and the slot plan

namespace {

constexpr int XV_AGREE_THREADS = 512;  // of the fused form (whole waves; the staging helpers are called by the first 256)
constexpr int XV_AGREE_MAX_GRID = 512;

// cell of one pixel inside its group's slice: ((label 2^E + mask) 2 + unanimous) 3 + outcome from the E labels packed in `key`
// (5 bits each, l_0 in the highest place), the ground truth l (0 <= l < C) and the fused label
__device__ static __forceinline__ int agreement_cell(int key, int E, int l, int fused) {
  const int l0 = (key >> (5 * (E - 1))) & 31;
  int mask = 0;
  bool same = true, hit = false;
#pragma unroll
  for (int e = 0; e < XV_MULTI_MAXE; ++e)
    if (e < E) {
      const int le = (key >> (5 * (E - 1 - e))) & 31;
      mask |= (le == l ? 1 : 0) << e;
      same = same && le == l0;
      hit = hit || le == fused;
    }
  const int outcome = fused == l ? 0 : (hit ? 1 : 2);
  return (((l << E) + mask) * 2 + (same ? 1 : 0)) * 3 + outcome;
}

// one workgroup's counters of one image into its group's slice; every thread of the workgroup calls it between two barriers
__device__ static __forceinline__ void agreement_flush(const uint32_t* cnt, int cells, unsigned long long* dst) {
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    const uint32_t v = cnt[i];
    if (v) atomicAdd(&dst[i], (unsigned long long)v);
  }
}

template <int CM, int MODE>
__global__ __launch_bounds__(XV_AGREE_THREADS) void fused_head_multi_agreement_kernel(
    HeadPtrs ptrs, int E, int N, int Hi, int Wi, int C, const float* __restrict__ tab_g, const float* __restrict__ lognorm_g,
    const float* __restrict__ logprior_g, const int32_t* __restrict__ labels, const int32_t* __restrict__ group, int NG,
    int parts, unsigned long long* __restrict__ table) {
  extern __shared__ __attribute__((aligned(16))) float ag_tab[];
  const int rows = MODE == 1 ? CM : C;  // table rows per expert
  const int ntab = MODE == 2 ? 0 : E * rows * CM + (MODE == 1 ? E * CM : 0) + CM;
  float* ln = ag_tab + E * rows * CM;             // [E][CM], Dirichlet only
  float* lp = ln + (MODE == 1 ? E * CM : 0);      // [CM]
  uint32_t* cnt = reinterpret_cast<uint32_t*>(ag_tab + ntab);  // [C][2^E][2][3]
  const int cells = (C << E) * 6;
  if (threadIdx.x < 256) {  // (the staging helpers stride by 256)
    if constexpr (MODE == 0) fuse_stage_rows<CM>(ag_tab, tab_g, E * C, C);
    if constexpr (MODE == 1) fuse_stage_dirichlet<CM>(ag_tab, ln, tab_g, lognorm_g, E, C);
    if constexpr (MODE != 2) fuse_stage_rows<CM>(lp, logprior_g, 1, C);
  }
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t ppi = (int64_t)Ho * Wo;  // pixels of one image
  const int64_t slots = (int64_t)N * parts;
  for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const int img = (int)(slot / parts), part = (int)(slot - (int64_t)img * parts);
    const int grp = group != nullptr ? group[img] : 0;
    if (grp < 0 || grp >= NG) continue;  // (uniform over the workgroup)
    for (int i = threadIdx.x; i < cells; i += XV_AGREE_THREADS) cnt[i] = 0u;
    __syncthreads();  // (the first one also publishes the tables)
    for (int64_t base = (int64_t)part * XV_AGREE_THREADS; base < ppi; base += (int64_t)parts * XV_AGREE_THREADS) {
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
      // running state over the experts: their labels in one word, 5 bits each, l_0 first; Dirichlet and mean: the sum
      constexpr int NT = MODE == 0 ? 1 : CM;
      float total[NT];
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
        const float m = head_max<CM>(sc, C);
        int le;
        if constexpr (MODE == 0) {
          le = head_label_fast<CM>(sc, m, C);
          if (le < 0) le = head_softmax<CM>(sc, m, C);
        } else if constexpr (MODE == 2) {
          le = head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
#pragma unroll
          for (int k = 0; k < CM; ++k) total[k] = e == 0 ? sc[k] : total[k] + sc[k];
        } else {
          le = head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
          fuse_renorm_log<CM, true>(sc, C);
          // the fmaf chain over k of dirichlet_fuse_kernel per class, two classes per v_pk_fma_f32 on the transposed table
          // (padded classes / terms are exact zeros: fma(0, 0, d) = d), as fused_head_multi_kernel
          f32x2 dot2[CM / 2];
#pragma unroll
          for (int cp = 0; cp < CM / 2; ++cp) dot2[cp] = f32x2{0.f, 0.f};
#pragma unroll
          for (int k = 0; k < CM; ++k) {
            const f32x2* rowk = reinterpret_cast<const f32x2*>(ag_tab + (e * CM + k) * CM);
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
        key = key * 32 + le;
      }
      int fused;
      if constexpr (MODE == 0) {
        // bayes_fuse_kernel: the E rows of the pixel's labels summed in ascending expert order
        float sc[CM];
#pragma nounroll
        for (int e = 0; e < E; ++e) {
          const int le = (key >> (5 * (E - 1 - e))) & 31;
          const f32x4* row = reinterpret_cast<const f32x4*>(ag_tab + (e * C + le) * CM);
#pragma unroll
          for (int k4 = 0; k4 < CM / 4; ++k4) {
            const f32x4 r = row[k4];
            sc[4 * k4] = e == 0 ? r.x : sc[4 * k4] + r.x;
            sc[4 * k4 + 1] = e == 0 ? r.y : sc[4 * k4 + 1] + r.y;
            sc[4 * k4 + 2] = e == 0 ? r.z : sc[4 * k4 + 2] + r.z;
            sc[4 * k4 + 3] = e == 0 ? r.w : sc[4 * k4 + 3] + r.w;
          }
        }
        fused = fuse_argmax_prior<CM>(sc, lp, C);
      } else if constexpr (MODE == 1) {
        fused = fuse_argmax_prior<CM>(total, lp, C);
      } else {
        fused = fuse_argmax_mean<CM>(total, (float)E, C);
      }
      xv_wave_count(cnt, valid ? agreement_cell(key, E, l, fused) : -1);
    }
    __syncthreads();
    agreement_flush(cnt, cells, table + (int64_t)grp * cells);
    __syncthreads();  // (the next slot clears the counters)
  }
}

// The same table from materialised maps: labels int32, the experts' and the fused labels int64, [n][ppi] each.  The cell
// depends on comparisons of the map values alone (and on the checked ground truth), so whatever a map holds stays in bounds.
struct AgreementMaps {
  const int64_t* p[XV_MULTI_MAXE];
};

__device__ static __forceinline__ const int64_t* agreement_map(const AgreementMaps& m, int e) {
  return e == 0 ? m.p[0] : (e == 1 ? m.p[1] : (e == 2 ? m.p[2] : m.p[3]));
}

__global__ __launch_bounds__(1024) void agreement_table_kernel(const int32_t* __restrict__ labels, AgreementMaps maps, int E,
                                                              const int64_t* __restrict__ fused,
                                                              const int32_t* __restrict__ group, int N, int64_t ppi, int C,
                                                              int NG, int parts, unsigned long long* __restrict__ table) {
  extern __shared__ __attribute__((aligned(16))) uint32_t at_cnt[];  // [C][2^E][2][3]
  const int cells = (C << E) * 6;
  const int T = blockDim.x;
  const int64_t slots = (int64_t)N * parts;
  for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const int img = (int)(slot / parts), part = (int)(slot - (int64_t)img * parts);
    const int grp = group != nullptr ? group[img] : 0;
    if (grp < 0 || grp >= NG) continue;  // (uniform over the workgroup)
    for (int i = threadIdx.x; i < cells; i += T) at_cnt[i] = 0u;
    __syncthreads();
    for (int64_t base = (int64_t)part * T; base < ppi; base += (int64_t)parts * T) {
      const bool live = base + threadIdx.x < ppi;
      if (__ballot(live) == 0) continue;  // (wave-uniform)
      const int64_t at = (int64_t)img * ppi + (live ? base + threadIdx.x : ppi - 1);
      const int l = live ? labels[at] : -1;
      const int64_t f = fused[at];
      const int64_t l0 = maps.p[0][at];
      int mask = 0;
      bool same = true, hit = false;
#pragma unroll
      for (int e = 0; e < XV_MULTI_MAXE; ++e)
        if (e < E) {
          const int64_t le = agreement_map(maps, e)[at];
          mask |= (le == (int64_t)l ? 1 : 0) << e;
          same = same && le == l0;
          hit = hit || le == f;
        }
      const int outcome = f == (int64_t)l ? 0 : (hit ? 1 : 2);
      const bool valid = l >= 0 && l < C;
      xv_wave_count(at_cnt, valid ? (((l << E) + mask) * 2 + (same ? 1 : 0)) * 3 + outcome : -1);
    }
    __syncthreads();
    agreement_flush(at_cnt, cells, table + (int64_t)grp * cells);
    __syncthreads();  // (the next slot clears the counters)
  }
}

}  // namespace

extern "C" int xv_fused_head_multi_agreement_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi,
                                                 int wi, int num_classes, int mode, const float* tab, const float* lognorm,
                                                 const float* logprior, const int32_t* labels, const int32_t* group,
                                                 int num_groups, int64_t* table, int max_workgroups, void* stream) {
  XV_CHECK_ARG(labels && table && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)table & 7) == 0);
  XV_CHECK_ARG(xv_mode_tables_ok(mode, tab, lognorm, logprior) && xv_group_ok(group, num_groups) && max_workgroups >= 0);
  HeadPtrs ptrs;
  XV_CHECK_OK(xv_multi_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs));
  const int64_t ppi = (int64_t)hi * wi * 64;  // one image's pixels
  // two 512-thread workgroups per CU, never above 512, or the caller's bound
  XvSlotPlan plan;
  XV_CHECK_OK(xv_slot_plan(ppi, XV_AGREE_THREADS, ppi, n, xv_grid_bound(2, XV_AGREE_MAX_GRID, max_workgroups), plan));
  const size_t lds = (xv_multi_table_floats(mode, num_experts, num_classes) + ((size_t)num_classes << num_experts) * 6) * 4;
  hipStream_t s = (hipStream_t)stream;
#define XV_AG_MODE(CMV, MODE)                                                                                                \
  hipLaunchKernelGGL((fused_head_multi_agreement_kernel<CMV, MODE>), dim3(plan.grid), dim3(XV_AGREE_THREADS), lds, s, ptrs,   \
                     num_experts, n, hi, wi, num_classes, tab, lognorm, logprior, labels, group, num_groups, plan.parts,     \
                     reinterpret_cast<unsigned long long*>(table))
#define XV_AG(CMV) XV_MODE_SWITCH(mode, XV_AG_MODE, CMV)
  XV_CM_SWITCH(num_classes, XV_AG)
#undef XV_AG
#undef XV_AG_MODE
  return xv_launch_status();
}

extern "C" int xv_agreement_table(const int32_t* labels, const int64_t* const* expert_labels, int num_experts,
                                  const int64_t* fused, const int32_t* group, int n, int64_t ppi, int num_classes,
                                  int num_groups, int64_t* table, void* stream) {
  XV_CHECK_ARG(labels && expert_labels && fused && table && n >= 1 && ppi >= 1);
  XV_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)fused & 7) == 0 && ((uintptr_t)table & 7) == 0);
  XV_CHECK_ARG(xv_experts_classes_ok(num_experts, num_classes) && xv_group_ok(group, num_groups));
  AgreementMaps maps;
  XV_CHECK_ARG(xv_fill_expert_slots(expert_labels, num_experts, 7, maps.p));
  XV_CHECK_SHAPE(ppi <= ((int64_t)1 << 40) / n);
  // one 16-wave workgroup per CU, never above 512, as xv_confusion_matrix_grouped
  XvSlotPlan plan;
  XV_CHECK_OK(xv_slot_plan(ppi, 1024, ppi, n, xv_grid_bound(1, XV_AGREE_MAX_GRID, 0), plan));
  const size_t lds = ((size_t)num_classes << num_experts) * 6 * 4;
  hipLaunchKernelGGL(agreement_table_kernel, dim3(plan.grid), dim3(1024), lds, (hipStream_t)stream, labels, maps, num_experts,
                     fused, group, n, ppi, num_classes, num_groups, plan.parts, reinterpret_cast<unsigned long long*>(table));
  return xv_launch_status();
}
