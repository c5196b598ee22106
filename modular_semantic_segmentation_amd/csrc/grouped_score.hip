// Grouped scoring for gfx950: the counting kernels of score() with one more leading index, the GROUP of the image a pixel
// belongs to (a sequence, or the image itself), so that one pass over a test set leaves a confusion matrix per group
// (experiments/evaluation.py:42-55 scores a network once per sequence; a paired bootstrap needs a matrix per image).
//   xv_confusion_matrix_grouped           cm[group[i]][label][pred] += 1            (xv_confusion_matrix per group)
//   xv_fused_head_joint_hist_grouped_fwd  hist[group[i]][label][a][b] += 1          (xv_fused_head_joint_hist_fwd per group)
// Both deal out (image, part) slots to workgroups (xv_multi.h: xv_slot_plan, with the bounded grid); while images x parts fit
// the bound -- every batch size the models run -- a workgroup has exactly one slot and flushes once.  The group ids are read
// from device memory and checked before anything is indexed with them: an id outside [0, G) counts nothing.
#include "xv_common.h"
#include "xv_heads.h"  // the heads' per-pixel pieces (sets `fp contract(on)` for what follows, as heads.hip has it)
#include "xv_multi.h"  // the host side: the grid bound and the slot plan

namespace {

// copies of a [cells] u32 table that fit 64 KB of LDS, a power of two <= 32: the replication confusion_kernel (fusion.hip) uses
inline int grouped_table_copies(size_t cells) {
  int rep = 32;
  while (rep > 1 && cells * rep * 4 > 64 * 1024) rep >>= 1;
  return rep;
}

// base_model.py:136-151 per group.  confusion_kernel's counting: `XV_REP` u32 copies of the [C][C] table in LDS, copy = lane &
// (XV_REP - 1) in the fastest-varying position (one conflict-free ds_add_u32 per pixel whatever the labels are), four pixels
// per thread and step through 16-byte loads where `vec` says every image starts 16-byte aligned in both maps.  Part p of an
// image takes the steps p, p + parts, ... of its pixels.
__global__ __launch_bounds__(1024) void confusion_grouped_kernel(const int32_t* __restrict__ labels,
                                                                const int64_t* __restrict__ pred,
                                                                const int32_t* __restrict__ group, int N, int64_t ppi, int C,
                                                                int G, int parts, unsigned long long* __restrict__ cm, int XV_REP,
                                                                int vec) {
  extern __shared__ unsigned int gcm_cnt[];  // [C * C][XV_REP]
  const int T = blockDim.x;
  const int rep = threadIdx.x & (XV_REP - 1);
  auto count = [&](int l, int64_t p) {
    if (l >= 0 && l < C && p >= 0 && p < C) atomicAdd(&gcm_cnt[(l * C + (int)p) * XV_REP + rep], 1u);
  };
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  typedef long long i64x2 __attribute__((ext_vector_type(2)));
  const int64_t slots = (int64_t)N * parts, stride = (int64_t)parts * T;
  for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const int img = (int)(slot / parts), part = (int)(slot - (int64_t)img * parts);
    const int g = group[img];
    if (g < 0 || g >= G) continue;  // (uniform over the workgroup)
    for (int i = threadIdx.x; i < C * C * XV_REP; i += T) gcm_cnt[i] = 0u;
    __syncthreads();
    const int32_t* lab = labels + (int64_t)img * ppi;
    const int64_t* prd = pred + (int64_t)img * ppi;
    const int64_t quads = vec ? ppi >> 2 : 0, first = (int64_t)part * T + threadIdx.x;
    for (int64_t q = first; q < quads; q += stride) {
      const i32x4 l = *reinterpret_cast<const i32x4*>(lab + 4 * q);
      const i64x2 p0 = *reinterpret_cast<const i64x2*>(prd + 4 * q), p1 = *reinterpret_cast<const i64x2*>(prd + 4 * q + 2);
      count(l.x, p0.x);
      count(l.y, p0.y);
      count(l.z, p1.x);
      count(l.w, p1.y);
    }
    // the tail of the vector form / the whole image where an image does not start 16-byte aligned
    for (int64_t pix = 4 * quads + first; pix < ppi; pix += stride) count(lab[pix], prd[pix]);
    __syncthreads();
    unsigned long long* dst = cm + (int64_t)g * C * C;
    for (int i = threadIdx.x; i < C * C; i += T) {
      unsigned long long a = 0ull;
      for (int r = 0; r < XV_REP; ++r) a += gcm_cnt[i * XV_REP + r];
      if (a) atomicAdd(&dst[i], a);
    }
    __syncthreads();  // (the next slot clears the counters)
  }
}

// fused_head_joint_hist_kernel (heads.hip) per group: the experts' labels by the same device functions in the same order --
// head_load_taps / head_eval_taps / head_max / head_label_fast, head_softmax when that returns -1 -- on the same P consecutive
// output pixels per thread, u32 counters [C][C][C] in LDS through xv_wave_count.  Part p of an image takes the steps p, p +
// parts, ... of its pixel groups; the trip count is uniform over the workgroup (xv_wave_count needs whole waves; a lane past
// the end recomputes the image's last group and counts nothing).
template <int CM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CM <= 16 ? 4 : 1))) void fused_head_joint_hist_grouped_kernel(
    const float* __restrict__ Sa, const float* __restrict__ Sb, const float* __restrict__ ba, const float* __restrict__ bb, int N,
    int Hi, int Wi, int C, const int32_t* __restrict__ labels, const int32_t* __restrict__ group, int G, int parts,
    unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t gjh_cnt[];  // [C][C][C]
  const int cells = C * C * C;
  constexpr int P = xv_joint_hist_pixels(CM);
  const int Ho = Hi * 8, Wo = Wi * 8, Wq = Wo / P;
  const int64_t nquads = (int64_t)Ho * Wq;  // of one image
  const int64_t slots = (int64_t)N * parts;
  for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const int img = (int)(slot / parts), part = (int)(slot - (int64_t)img * parts);
    const int g = group[img];
    if (g < 0 || g >= G) continue;  // (uniform over the workgroup)
    for (int i = threadIdx.x; i < cells; i += 256) gjh_cnt[i] = 0u;
    __syncthreads();
    for (int64_t base = (int64_t)part * 256; base < nquads; base += (int64_t)parts * 256) {
      const bool live = base + threadIdx.x < nquads;
      const int64_t quad = live ? base + threadIdx.x : nquads - 1;
      const int ox0 = (int)(quad % Wq) * P;
      const int oy = (int)(quad / Wq);
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
        // (the second expert's taps wait for the first one's labels, as in fused_head_joint_hist_kernel)
        int ne = img;
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
      const i32xP lv = *reinterpret_cast<const i32xP*>(labels + ((int64_t)img * nquads + quad) * P);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int l = lv[p];
        xv_wave_count(gjh_cnt, (live && l >= 0 && l < C) ? (l * C + lab[0][p]) * C + lab[1][p] : -1);
      }
    }
    __syncthreads();
    unsigned long long* dst = hist + (int64_t)g * cells;
    for (int i = threadIdx.x; i < cells; i += 256) {
      const uint32_t v = gjh_cnt[i];
      if (v) atomicAdd(&dst[i], (unsigned long long)v);
    }
    __syncthreads();  // (the next slot clears the counters)
  }
}

}  // namespace

extern "C" int xv_confusion_matrix_grouped(const int32_t* labels, const int64_t* pred, const int32_t* group, int n, int64_t ppi,
                                           int num_classes, int num_groups, int64_t* cm, void* stream) {
  XV_CHECK_ARG(labels && pred && group && cm && n >= 1 && ppi >= 1 && num_groups >= 1);
  XV_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)group & 3) == 0 && ((uintptr_t)pred & 7) == 0 && ((uintptr_t)cm & 7) == 0);
  XV_CHECK_SHAPE(num_classes >= 1 && num_classes <= 64 && ppi <= ((int64_t)1 << 40) / n);
  const int rep = grouped_table_copies((size_t)num_classes * num_classes);
  const size_t lds = (size_t)num_classes * num_classes * rep * 4;  // 18 KB at C = 12
  // every image starts 16-byte aligned in both maps: whole label quads per image
  const int vec = ((uintptr_t)labels & 15) == 0 && ((uintptr_t)pred & 15) == 0 && (ppi & 3) == 0;
  // one 16-wave workgroup per CU, as xv_confusion_matrix; at most the 512 of the rule for kernels that end in such atomics
  XvSlotPlan plan;  // (a thread takes four pixels a step)
  XV_CHECK_OK(xv_slot_plan((ppi + 3) / 4, 1024, ppi, n, xv_grid_bound(1, 512, 0), plan));
  hipLaunchKernelGGL(confusion_grouped_kernel, dim3(plan.grid), dim3(1024), lds, (hipStream_t)stream, labels, pred, group, n,
                     ppi, num_classes, num_groups, plan.parts, reinterpret_cast<unsigned long long*>(cm), rep, vec);
  return xv_launch_status();
}

extern "C" int xv_fused_head_joint_hist_grouped_fwd(const float* Sa, const float* Sb, const float* bias_a, const float* bias_b,
                                                    int n, int hi, int wi, int num_classes, const int32_t* labels,
                                                    const int32_t* group, int num_groups, int64_t* hist, int max_workgroups,
                                                    void* stream) {
  XV_CHECK_ARG(Sa && Sb && bias_a && bias_b && labels && group && hist && ((uintptr_t)labels & 15) == 0);
  XV_CHECK_ARG(((uintptr_t)group & 3) == 0 && ((uintptr_t)hist & 7) == 0 && num_groups >= 1);
  XV_CHECK_ARG(num_classes >= 2 && num_classes <= 20 && max_workgroups >= 0);  // 20^3 u32 counters: 32 KB of LDS
  XV_CHECK_SHAPE(xv_dims_sane(n, hi, wi));
  const int64_t nquads = (int64_t)hi * wi * 64 / xv_joint_hist_pixels((num_classes + 3) / 4 * 4);  // one image's pixel groups
  // four 256-thread workgroups per CU as the ungrouped head, or the caller's bound
  XvSlotPlan plan;  // (a pixel group adds at most four to a counter)
  XV_CHECK_OK(xv_slot_plan(nquads, 256, nquads * 4, n, xv_grid_bound(4, 0, max_workgroups), plan));
  const size_t lds = (size_t)num_classes * num_classes * num_classes * 4;
  hipStream_t s = (hipStream_t)stream;
#define XV_GJH(CMV)                                                                                                          \
  hipLaunchKernelGGL(fused_head_joint_hist_grouped_kernel<CMV>, dim3(plan.grid), dim3(256), lds, s, Sa, Sb, bias_a, bias_b, n, \
                     hi, wi, num_classes, labels, group, num_groups, plan.parts, reinterpret_cast<unsigned long long*>(hist))
  switch ((num_classes + 3) / 4) {  // (XV_CM_SWITCH up to the 20 classes this entry point takes: nothing is built beyond)
    case 1: XV_GJH(4); break;
    case 2: XV_GJH(8); break;
    case 3: XV_GJH(12); break;
    case 4: XV_GJH(16); break;
    default: XV_GJH(20); break;
  }
#undef XV_GJH
  return xv_launch_status();
}
