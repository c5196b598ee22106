// Counting form of the fused head for two to four experts, gfx950: fused_head_multi_kernel (heads.hip) with the confusion
// matrix counted in place of the label map, under G parameter sets at once and, where asked, per GROUP of images -- what
// fused_head_grid_score_kernel / fused_head_joint_hist_kernel / fused_head_average_kernel<COUNT> (heads.hip) and
// fused_head_joint_hist_grouped_kernel (grouped_score.hip) are for two experts.  A joint histogram of the experts' labels does
// not extend (C^(E+1) counters), fusing the pixel under every parameter set and counting in LDS does.
//
// Per output pixel and expert ONCE, ascending expert order, statement for statement as fused_head_multi_kernel (written
// out here, not through xv_fuse.h: see there):
// head_load_taps / head_eval_taps / head_max, then
//   MODE 0, Bayes      head_label_fast, head_softmax when it returns -1; after the experts the row sum
//                      ((tab_0[l_0][k] + tab_1[l_1][k]) + ...) once, and per point + logprior_g[k], first maximum
//                      (bayes_fuse_kernel's order: the label of the predict-side kernel whether it took its decision table
//                      or its row sums; the log-likelihood tables are shared by all points, only the prior is searched)
//   MODE 1, Dirichlet  head_softmax, renormalise, log(1e-20 + p), kept for every expert; per point the ascending-k fmaf chains on
//                      the transposed table (two classes per v_pk_fma_f32), - lognorm, total = L_0, += L_1, ..., + logprior,
//                      first maximum (dirichlet_fuse_kernel's order)
//   MODE 2, mean       head_softmax, s = ((p_0 + p_1) + ...), v = s / E (IEEE division), first maximum; one point
// so fused_g is the label xv_fused_head_multi_fwd writes with point g's tables, bit for bit, and the expert's own label l_e
// (head_softmax's, or head_label_fast's where that decides: the same label) is the one decoder_head_kernel stores.
// cm[group][g][label][fused_g] += 1 and, where expert_cm is given, expert_cm[group][e][label][l_e] += 1 over the pixels with
// 0 <= label < C.
//
// One pixel per thread, as the Dirichlet grid-scoring head.  MODE 0 and 2 run the experts in a rolled loop on running state
// (the labels packed into one word; the sum [CM]), EU = 0: one instantiation for every expert count.  MODE 1 keeps E x CM
// log-probabilities, which a rolled loop would have to index by a run-time expert number: it is instantiated per expert
// count, EU = 2, 3, 4, and unrolled.
//
// Work is dealt out in (image, part) slots (xv_multi.h: xv_slot_plan), counted through xv_wave_count; the trip count is
// uniform over the workgroup (xv_wave_count needs whole waves; a lane past the end recomputes the image's last pixel and counts
// nothing).  The grid is bounded (four workgroups per CU, or the caller's bound).  group == nullptr: every image is group 0.
// A group id is checked before anything is indexed with it: outside [0, NG) counts nothing.
//
// LDS of one launch, 40 KB at most (four workgroups per CU, as the grid-scoring heads of heads.hip), in this order:
//   MODE 0   tab [E][C][CM], logprior [G][CM]
//   MODE 1   per point: tab [E][CM k][CM c] (transposed), lognorm [E][CM], logprior [CM]
//   then u32 counters [G][C][C] and, with expert_cm, [E][C][C].
// xv_fused_head_multi_count_capacity always leaves room for the expert counters.  32 classes and four experts hold one point in
// every mode within the 40 KB (Dirichlet: 17 024 B of tables + 4 096 + 16 384 B of counters), so no case raises the budget.
#include <stdlib.h>

#include "xv_common.h"
#include "xv_heads.h"  // the heads' per-pixel pieces (sets `fp contract(on)` for what follows, as heads.hip has it)
#include "xv_multi.h"  // the host side: argument checks and the slot plan

namespace {

constexpr size_t XV_MULTI_COUNT_LDS = 40 * 1024;

// waves per SIMD the register allocation is held to.  Bayes and mean: the two-expert counting heads' four up to 16 classes.
// Dirichlet holds (EU - 1) CM log-probabilities beside the 4 CM taps and the CM scores of the expert in work, (EU + 4) CM in
// all before any address, weight or dot product: four waves (128 registers) while that leaves 32, then three (168), two (256).
// Four experts need one step more than that rule gives (12 classes: 472 bytes of scratch at four waves, none at three).
constexpr int xv_count_waves(int cm, int mode, int eu) {
  if (mode != 1) return cm <= 16 ? 4 : 1;
  const int live = (eu + 4) * cm + (eu == 4 ? 48 : 32);
  return live <= 128 ? 4 : (live <= 168 ? 3 : (live <= 256 ? 2 : 1));
}

// Four experts at 24 classes and more: the taps of a whole expert (4 CM registers) beside three experts' log-probabilities
// and the scores in work pass the 256 registers a lane can address, so there the taps are loaded and evaluated one class quad
// at a time (16 registers: head_logits_quads, xv_heads.h).
constexpr bool xv_count_quads(int cm, int eu) { return eu == 4 && cm >= 24; }

template <int CM, int MODE, int EU>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(xv_count_waves(CM, MODE, EU)))) void fused_head_multi_count_kernel(
    HeadPtrs ptrs, int E_, int N, int Hi, int Wi, int C, int G, const float* __restrict__ tab_g,
    const float* __restrict__ lognorm_g, const float* __restrict__ logprior_g, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ group, int NG, int parts, unsigned long long* __restrict__ cm,
    unsigned long long* __restrict__ ecm) {
  static_assert(MODE == 1 ? (EU >= 2 && EU <= XV_MULTI_MAXE) : EU == 0, "Dirichlet per expert count, the others rolled");
  const int E = EU > 0 ? EU : E_;
  constexpr int NE = EU > 0 ? EU : 1;          // (array extents of the Dirichlet form)
  const int PT = E * CM * CM + E * CM + CM;    // floats per Dirichlet point
  extern __shared__ __attribute__((aligned(16))) float mc_tab[];
  const int ntab = MODE == 0 ? E * C * CM + G * CM : (MODE == 1 ? G * PT : 0);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(mc_tab + ntab);  // [G][C][C]
  const int ncnt = G * C * C;
  uint32_t* ecnt = cnt + ncnt;  // [E][C][C]
  const int necnt = ecm != nullptr ? E * C * C : 0;
  if constexpr (MODE == 0) {
    for (int i = threadIdx.x; i < E * C * CM; i += 256) {
      const int k = i % CM, row = i / CM;
      mc_tab[i] = k < C ? tab_g[row * C + k] : 0.f;
    }
    float* lpr = mc_tab + E * C * CM;
    for (int i = threadIdx.x; i < G * CM; i += 256) {
      const int k = i % CM, g = i / CM;
      lpr[i] = k < C ? logprior_g[g * C + k] : 0.f;
    }
  }
  if constexpr (MODE == 1) {
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
      mc_tab[i] = v;
    }
  }
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t ppi = (int64_t)Ho * Wo;  // pixels of one image
  const int64_t slots = (int64_t)N * parts;
  for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const int img = (int)(slot / parts), part = (int)(slot - (int64_t)img * parts);
    const int grp = group != nullptr ? group[img] : 0;
    if (grp < 0 || grp >= NG) continue;  // (uniform over the workgroup)
    for (int i = threadIdx.x; i < ncnt + necnt; i += 256) cnt[i] = 0u;
    __syncthreads();  // (the first one also publishes the tables)
    for (int64_t base = (int64_t)part * 256; base < ppi; base += (int64_t)parts * 256) {
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
      if constexpr (MODE == 1) {
        f32x2 lg[NE][CM / 2];  // log(1e-20 + p) of every expert, class pairs (the splat of one class is an operand modifier)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          // an expert's taps are requested after the arithmetic of the one before (its address waits for a result of it: an
          // empty asm, no instruction): left alone the scheduler asks for several sets of taps, 4 CM registers each, at once
          int ne = img;
          if (e > 0) asm volatile("" : "+v"(ne) : "v"(lg[e > 0 ? e - 1 : 0][CM / 2 - 1].y));
          float sc[CM];
          if constexpr (xv_count_quads(CM, EU)) {
            head_logits_quads<CM>(ptrs.s[e], ptrs.b[e], ne, iy1, ix1, Hi, Wi, wy1, wy0, wx1, wx0, C, sc);
          } else {
            f32x4 ta[CM / 4], tb[CM / 4], tc[CM / 4], td[CM / 4];
            head_load_taps<CM>(ptrs.s[e], ne, iy1, ix1, Hi, Wi, ta, tb, tc, td);
            head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, ptrs.b[e], C, sc);
          }
          const float m = head_max<CM>(sc, C);
          const int le = head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
          if (ecm != nullptr) xv_wave_count(ecnt + e * C * C, valid ? l * C + le : -1);
          float sum = 0.f;  // (fuse_renorm_log of xv_fuse.h, written out: through it this kernel measured slower, see there)
#pragma unroll
          for (int k = 0; k < CM; ++k) {
            sc[k] = k < C ? sc[k] : 0.f;
            sum += sc[k];
          }
          const float rs = xv_fast_rcp(sum);
#pragma unroll
          for (int k = 0; k < CM; ++k) sc[k] = k < C ? xv_fast_log(1e-20f + sc[k] * rs) : 0.f;  // renormalise, then log(1e-20 + p)
#pragma unroll
          for (int k2 = 0; k2 < CM / 2; ++k2) lg[e][k2] = f32x2{sc[2 * k2], sc[2 * k2 + 1]};
        }
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
          const float* tg = mc_tab + g * PT;
          const float* ln = tg + NE * CM * CM;
          const float* lp = ln + NE * CM;
          // four classes at a time, every expert's dot products side by side: nothing of size CM but lg stays live
          float best = 0.f;
          int bi = 0, toff = 0;
#pragma unroll
          for (int c4 = 0; c4 < CM / 4; ++c4) {
            f32x2 dot2[NE][2];
#pragma unroll
            for (int e = 0; e < NE; ++e) {
              dot2[e][0] = dot2[e][1] = f32x2{0.f, 0.f};
              // (the wide four-expert forms: the class splats of lg are formed where they are used -- redefined here by an empty
              // asm, no instruction -- and not once for all points and class quads, which is 2 E CM registers more)
              if constexpr (xv_count_quads(CM, EU)) {
#pragma unroll
                for (int k2 = 0; k2 < CM / 2; ++k2) asm volatile("" : "+v"(lg[e][k2]));
              }
#pragma unroll
              for (int k = 0; k < CM; ++k) {
                // (the wide four-expert forms: at most eight table rows in flight beside the 4 CM log-probabilities; no instruction)
                if constexpr (xv_count_quads(CM, EU))
                  if (k % 8 == 0 && (e > 0 || k > 0)) asm volatile("" : "+v"(toff) : "v"(dot2[k > 0 ? e : (e > 0 ? e - 1 : 0)][1].y));
                const f32x4 r = *reinterpret_cast<const f32x4*>(tg + toff + (e * CM + k) * CM + 4 * c4);
                const f32x2 lk = (k & 1) ? lg[e][k >> 1].yy : lg[e][k >> 1].xx;
                dot2[e][0] = __builtin_elementwise_fma(f32x2{r.x, r.y}, lk, dot2[e][0]);
                dot2[e][1] = __builtin_elementwise_fma(f32x2{r.z, r.w}, lk, dot2[e][1]);
              }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int c = 4 * c4 + j;
              float total = dot2[0][j >> 1][j & 1] - ln[c];
#pragma unroll
              for (int e = 1; e < NE; ++e) {
                const float L = dot2[e][j >> 1][j & 1] - ln[e * CM + c];
                total = total + L;
              }
              const float v = total + lp[c];
              if (c < C && (c == 0 || v > best)) {
                best = v;
                bi = c;
              }
            }
          }
          xv_wave_count(cnt + g * C * C, valid ? l * C + bi : -1);
        }
      } else {
        // running state over the experts.  Bayes: the pixel's expert labels in one word, 5 bits each, l_0 first; mean: the sum
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
            key = key * 32 + le;
          } else {
            le = head_softmax<CM>(sc, m, C);  // sc = the probabilities the unfused path stores
#pragma unroll
            for (int k = 0; k < CM; ++k) total[k] = e == 0 ? sc[k] : total[k] + sc[k];
          }
          if (ecm != nullptr) xv_wave_count(ecnt + e * C * C, valid ? l * C + le : -1);
        }
        if constexpr (MODE == 0) {
          // bayes_fuse_kernel: the E rows of the pixel's labels summed in ascending expert order, once for all points
          float sc[CM];
#pragma nounroll
          for (int e = 0; e < E; ++e) {
            const int le = (key >> (5 * (E - 1 - e))) & 31;
            const f32x4* row = reinterpret_cast<const f32x4*>(mc_tab + (e * C + le) * CM);
#pragma unroll
            for (int k4 = 0; k4 < CM / 4; ++k4) {
              const f32x4 r = row[k4];
              sc[4 * k4] = e == 0 ? r.x : sc[4 * k4] + r.x;
              sc[4 * k4 + 1] = e == 0 ? r.y : sc[4 * k4 + 1] + r.y;
              sc[4 * k4 + 2] = e == 0 ? r.z : sc[4 * k4 + 2] + r.z;
              sc[4 * k4 + 3] = e == 0 ? r.w : sc[4 * k4 + 3] + r.w;
            }
          }
          const float* lpr = mc_tab + E * C * CM;
#pragma unroll 1
          for (int g = 0; g < G; ++g) {
            const float* lp = lpr + g * CM;
            float best = 0.f;
            int bi = 0;
#pragma unroll
            for (int k = 0; k < CM; ++k) {
              const float v = sc[k] + lp[k];
              if (k < C && (k == 0 || v > best)) {
                best = v;
                bi = k;
              }
            }
            xv_wave_count(cnt + g * C * C, valid ? l * C + bi : -1);
          }
        } else {
          const float fe = (float)E;
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
          xv_wave_count(cnt, valid ? l * C + bi : -1);
        }
      }
    }
    __syncthreads();
    unsigned long long* dst = cm + (int64_t)grp * ncnt;
    for (int i = threadIdx.x; i < ncnt; i += 256) {
      const uint32_t v = cnt[i];
      if (v) atomicAdd(&dst[i], (unsigned long long)v);
    }
    if (necnt > 0) {
      unsigned long long* edst = ecm + (int64_t)grp * necnt;
      for (int i = threadIdx.x; i < necnt; i += 256) {
        const uint32_t v = ecnt[i];
        if (v) atomicAdd(&edst[i], (unsigned long long)v);
      }
    }
    __syncthreads();  // (the next slot clears the counters)
  }
}

// bytes of LDS every launch holds whatever its points are (the expert counters; Bayes: the shared tables), and per point
size_t multi_count_fixed_bytes(int num_classes, int num_experts, int mode) {
  const size_t c = (size_t)num_classes, cm = (c + 3) / 4 * 4, e = (size_t)num_experts;
  return (e * c * c + (mode == 0 ? e * c * cm : 0)) * 4;
}
size_t multi_count_point_bytes(int num_classes, int num_experts, int mode) {
  const size_t c = (size_t)num_classes, cm = (c + 3) / 4 * 4, e = (size_t)num_experts;
  return (c * c + (mode == 0 ? cm : (mode == 1 ? e * cm * cm + e * cm + cm : 0))) * 4;
}

}  // namespace

extern "C" int xv_fused_head_multi_count_capacity(int num_classes, int num_experts, int mode) {
  if (num_classes < 2 || num_classes > 32 || num_experts < 2 || num_experts > XV_MULTI_MAXE || mode < 0 || mode > 2) return 0;
  const size_t fixed = multi_count_fixed_bytes(num_classes, num_experts, mode);
  const size_t point = multi_count_point_bytes(num_classes, num_experts, mode);
  if (fixed + point > XV_MULTI_COUNT_LDS) return 0;
  return mode == 2 ? 1 : (int)((XV_MULTI_COUNT_LDS - fixed) / point);
}

extern "C" int xv_fused_head_multi_count_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi,
                                             int wi, int num_classes, int mode, int num_points, const float* tab,
                                             const float* lognorm, const float* logprior, const int32_t* labels,
                                             const int32_t* group, int num_groups, int64_t* cm, int64_t* expert_cm,
                                             int max_workgroups, void* stream) {
  XV_CHECK_ARG(labels && cm && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)cm & 7) == 0 && ((uintptr_t)expert_cm & 7) == 0);
  XV_CHECK_ARG(xv_mode_tables_ok(mode, tab, lognorm, logprior) && xv_group_ok(group, num_groups) && max_workgroups >= 0);
  XV_CHECK_ARG(num_points >= 1 && num_points <= xv_fused_head_multi_count_capacity(num_classes, num_experts, mode));
  HeadPtrs ptrs;
  XV_CHECK_OK(xv_multi_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs));
  const int64_t ppi = (int64_t)hi * wi * 64;  // one image's pixels
  // four 256-thread workgroups per CU as the two-expert counting heads, or the caller's bound
  XvSlotPlan plan;
  XV_CHECK_OK(xv_slot_plan(ppi, 256, ppi, n, xv_grid_bound(4, 0, max_workgroups), plan));
  const size_t lds = multi_count_point_bytes(num_classes, num_experts, mode) * num_points +
                     multi_count_fixed_bytes(num_classes, num_experts, mode) -
                     (expert_cm ? 0 : (size_t)num_experts * num_classes * num_classes * 4);
  hipStream_t s = (hipStream_t)stream;
#define XV_MC_MODE(CMV, MODE, EU)                                                                                            \
  hipLaunchKernelGGL((fused_head_multi_count_kernel<CMV, MODE, EU>), dim3(plan.grid), dim3(256), lds, s, ptrs, num_experts, \
                     n, hi, wi, num_classes, num_points, tab, lognorm, logprior, labels, group, num_groups, plan.parts,     \
                     reinterpret_cast<unsigned long long*>(cm), reinterpret_cast<unsigned long long*>(expert_cm))
#define XV_MC(CMV)                  \
  {                                 \
    if (mode == 0)                  \
      XV_MC_MODE(CMV, 0, 0);        \
    else if (mode == 2)             \
      XV_MC_MODE(CMV, 2, 0);        \
    else if (num_experts == 2)      \
      XV_MC_MODE(CMV, 1, 2);        \
    else if (num_experts == 3)      \
      XV_MC_MODE(CMV, 1, 3);        \
    else                            \
      XV_MC_MODE(CMV, 1, 4);        \
  }
  XV_CM_SWITCH(num_classes, XV_MC)
#undef XV_MC
#undef XV_MC_MODE
  return xv_launch_status();
}
