// Label-tuple heads for gfx950: what a fusion that sees a pixel ONLY through the tuple of its experts' labels needs from the
// experts' low-resolution class scores -- the histogram of the tuples (no ground truth: the data IBCC adapts on is unlabelled)
// and the decision through a lookup table over the tuples, written as a label map or counted against the ground truth.
//
// THE TUPLE.  E experts (2..4), C classes: t = ((l_0 C + l_1) C + l_2) ..., expert 0 most significant, T = C^E tuples: the
// row-major index of bayes_decision_matrix's [C]*E array.  l_e is the label decoder_head_kernel stores for expert e, bit for
// bit: per output pixel and expert, ascending expert order, head_load_taps / head_eval_taps / head_max, head_label_fast and
// head_softmax where that returns -1 -- the statements of fused_head_multi_kernel's Bayes mode (heads.hip), whose running
// word in radix C IS the tuple.  The experts run in a rolled loop: one instantiation per class step whatever the expert count.
//
//   xv_fused_head_multi_tuple_hist_fwd   hist[group][t] += 1 over EVERY output pixel
//   xv_fused_head_multi_lut_fwd          fused_label = lut[t]: four pixels per thread, two 16-byte stores, as the Bayes head
//   xv_fused_head_multi_lut_count_fwd    cm[group][label][lut[t]] += 1 over the pixels with 0 <= label < C; no label map
//
// The two counting kernels deal their work out in (image, part) slots (xv_multi.h: xv_slot_plan), counted through
// xv_wave_count, so a counter never wraps; the trip count is uniform over the workgroup (xv_wave_count needs whole waves; a
// lane past the end recomputes the image's last pixel and counts nothing).  The grid is bounded, at most 512 workgroups of
// 512 threads.  group == nullptr: every image is group 0.  A group id is checked before anything is indexed with it.
//
// LDS.  The histogram holds T u32 counters and nothing else; the counting lookup holds the table (T bytes, rounded up to 16)
// and C C u32 counters; the lookup head holds the table.  The histogram is the largest, so it sets what is served: 4 T bytes
// within the 160 KB of a gfx950 workgroup, T <= 40 960 -- every pair of two and three experts up to 32 classes, four experts
// up to 14 classes (12 classes: 20 736 tuples, 81 KB).  Above 64 KB a workgroup has a CU's LDS to itself: one 512-thread
// workgroup is two waves per SIMD, which is what these kernels are held to.
#include "xv_common.h"
#include "xv_heads.h"  // the heads' per-pixel pieces (sets `fp contract(on)` for what follows, as heads.hip has it)
#include "xv_multi.h"  // the host side: argument checks and the slot plan

namespace {

constexpr int XV_TUPLE_THREADS = 512;       // of the two counting kernels (whole waves)
constexpr int XV_TUPLE_MAX_GRID = 512;
constexpr int XV_TUPLE_LDS = 160 * 1024;    // one workgroup's LDS on gfx950
constexpr int64_t XV_TUPLE_MAX = XV_TUPLE_LDS / 4;  // tuples whose u32 counters fit it

// C^E, or 0 where the pair is not served
int64_t tuple_count(int num_classes, int num_experts) {
  if (num_classes < 2 || num_classes > 32 || num_experts < 2 || num_experts > XV_MULTI_MAXE) return 0;
  int64_t t = 1;
  for (int e = 0; e < num_experts; ++e) t *= num_classes;
  return t <= XV_TUPLE_MAX ? t : 0;
}

// the tuple of one output pixel: every expert's label in radix C, l_0 first
template <int CM>
__device__ static __forceinline__ int tuple_of_pixel(const HeadPtrs& ptrs, int E, int img, int iy1, int ix1, int Hi, int Wi,
                                                     float wy1, float wy0, float wx1, float wx0, int C) {
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
    int le = head_label_fast<CM>(sc, m, C);
    if (le < 0) le = head_softmax<CM>(sc, m, C);
    key = key * C + le;
  }
  return key;
}

// the lookup table into LDS, words first (lut_g is 4-byte aligned), then the tail; the caller synchronises
__device__ static __forceinline__ void tuple_stage_lut(uint8_t* lut, const uint8_t* __restrict__ lut_g, int T) {
  const int words = T >> 2;
  for (int i = threadIdx.x; i < words; i += blockDim.x)
    reinterpret_cast<uint32_t*>(lut)[i] = reinterpret_cast<const uint32_t*>(lut_g)[i];
  for (int i = (words << 2) + threadIdx.x; i < T; i += blockDim.x) lut[i] = lut_g[i];
}

// one workgroup's counters of one image into its group's slice; every thread of the workgroup calls it between two barriers
__device__ static __forceinline__ void tuple_flush(const uint32_t* cnt, int cells, unsigned long long* dst) {
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    const uint32_t v = cnt[i];
    if (v) atomicAdd(&dst[i], (unsigned long long)v);
  }
}

// COUNT false: the tuple histogram, cnt [T].  COUNT true: the table's decisions against the ground truth, lut [T] then cnt
// [C][C]; a table entry outside [0, C) counts nothing (it is never used as an index).
template <int CM, bool COUNT>
__global__ __launch_bounds__(XV_TUPLE_THREADS) void fused_head_multi_tuple_kernel(
    HeadPtrs ptrs, int E, int N, int Hi, int Wi, int C, int T, const uint8_t* __restrict__ lut_g,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ group, int NG, int parts,
    unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t tl_lds[];
  const int nlut = COUNT ? (T + 15) / 16 * 16 : 0;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(tl_lds + nlut);
  const int cells = COUNT ? C * C : T;
  if constexpr (COUNT) tuple_stage_lut(tl_lds, lut_g, T);
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t ppi = (int64_t)Ho * Wo;  // pixels of one image
  const int64_t slots = (int64_t)N * parts;
  for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
    const int img = (int)(slot / parts), part = (int)(slot - (int64_t)img * parts);
    const int grp = group != nullptr ? group[img] : 0;
    if (grp < 0 || grp >= NG) continue;  // (uniform over the workgroup)
    for (int i = threadIdx.x; i < cells; i += XV_TUPLE_THREADS) cnt[i] = 0u;
    __syncthreads();  // (the first one also publishes the table)
    for (int64_t base = (int64_t)part * XV_TUPLE_THREADS; base < ppi; base += (int64_t)parts * XV_TUPLE_THREADS) {
      const bool live = base + threadIdx.x < ppi;
      if (__ballot(live) == 0) continue;  // (wave-uniform)
      const int64_t pix = live ? base + threadIdx.x : ppi - 1;
      const int ox = (int)(pix % Wo);
      const int oy = (int)(pix / Wo);
      int iy1, ix1;
      float wy1, wy0, wx1, wx0;
      bilinear_taps<8>(oy, iy1, wy1, wy0);
      bilinear_taps<8>(ox, ix1, wx1, wx0);
      const int key = tuple_of_pixel<CM>(ptrs, E, img, iy1, ix1, Hi, Wi, wy1, wy0, wx1, wx0, C);
      if constexpr (COUNT) {
        const int l = live ? labels[(int64_t)img * ppi + pix] : -1;
        const int fused = tl_lds[key];
        xv_wave_count(cnt, (l >= 0 && l < C && fused < C) ? l * C + fused : -1);
      } else {
        xv_wave_count(cnt, live ? key : -1);
      }
    }
    __syncthreads();
    tuple_flush(cnt, cells, out + (int64_t)grp * cells);
    __syncthreads();  // (the next slot clears the counters)
  }
}

// fused_label = lut[t], four output pixels of one row per thread (they share their taps but for one column step, as
// fused_head_multi_kernel's Bayes mode) and two 16-byte stores; a workgroup stages the table once and walks the pixel quads
// grid-stride.
// waves per SIMD the register allocation is held to: four up to 12 classes (fused_head_multi_kernel's Bayes mode), never
// fewer than two
constexpr int xv_lut_waves(int cm) { return cm <= 12 ? 4 : 2; }

template <int CM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(xv_lut_waves(CM)))) void fused_head_multi_lut_kernel(
    HeadPtrs ptrs, int E, int N, int Hi, int Wi, int C, int T, const uint8_t* __restrict__ lut_g, int64_t* __restrict__ fused) {
  constexpr int P = 4;
  extern __shared__ __attribute__((aligned(16))) uint8_t lut[];
  tuple_stage_lut(lut, lut_g, T);
  __syncthreads();
  const int Ho = Hi * 8, Wo = Wi * 8, Wq = Wo / P;
  const int64_t nquads = (int64_t)N * Ho * Wq;
  for (int64_t quad = (int64_t)blockIdx.x * 256 + threadIdx.x; quad < nquads; quad += (int64_t)gridDim.x * 256) {
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
    int key[P];
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
        float sc[CM];
        head_eval_taps<CM>(ta, tb, tc, td, wy1, wy0, wx1, wx0, bs, C, sc);
        const float m = head_max<CM>(sc, C);
        int l = head_label_fast<CM>(sc, m, C);
        if (l < 0) l = head_softmax<CM>(sc, m, C);
        key[p] = key[p] * C + l;
      }
    }
    typedef __attribute__((ext_vector_type(2))) long long i64x2;
    int64_t* dst = fused + quad * P;
#pragma unroll
    for (int p = 0; p < P; p += 2) *reinterpret_cast<i64x2*>(dst + p) = i64x2{(long long)lut[key[p]], (long long)lut[key[p + 1]]};
  }
}

// the checks the three entry points share; on success ptrs holds the experts' pointers
int tuple_check_experts(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                        int num_classes, HeadPtrs& ptrs) {
  XV_CHECK_OK(xv_multi_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs));
  XV_CHECK_SHAPE(tuple_count(num_classes, num_experts) > 0);
  return XV_OK;
}

// both counting forms: the bounded grid, the parts of an image, the LDS above 64 KB allowed once per kernel and device
template <bool COUNT>
int tuple_launch(const HeadPtrs& ptrs, int num_experts, int n, int hi, int wi, int num_classes, const uint8_t* lut,
                 const int32_t* labels, const int32_t* group, int num_groups, int64_t* out, int max_workgroups,
                 hipStream_t s) {
  const int T = (int)tuple_count(num_classes, num_experts);
  const int64_t ppi = (int64_t)hi * wi * 64;  // one image's pixels
  // two 512-thread workgroups per CU where the LDS lets them, never above 512, or the caller's bound
  XvSlotPlan plan;
  XV_CHECK_OK(xv_slot_plan(ppi, XV_TUPLE_THREADS, ppi, n, xv_grid_bound(2, XV_TUPLE_MAX_GRID, max_workgroups), plan));
  const size_t lds = COUNT ? (size_t)(T + 15) / 16 * 16 + (size_t)num_classes * num_classes * 4 : (size_t)T * 4;
#define XV_TL(CMV)                                                                                                         \
  {                                                                                                                        \
    static bool attr[XV_MAX_DEVICES] = {false};                                                                            \
    const hipError_t e = xv_allow_dynamic_lds(reinterpret_cast<const void*>(&fused_head_multi_tuple_kernel<CMV, COUNT>),   \
                                              XV_TUPLE_LDS, attr, false);                                                  \
    if (e != hipSuccess) return (int)e;                                                                                    \
    hipLaunchKernelGGL((fused_head_multi_tuple_kernel<CMV, COUNT>), dim3(plan.grid), dim3(XV_TUPLE_THREADS), lds, s, ptrs,  \
                       num_experts, n, hi, wi, num_classes, T, lut, labels, group, num_groups, plan.parts,                 \
                       reinterpret_cast<unsigned long long*>(out));                                                        \
  }
  XV_CM_SWITCH(num_classes, XV_TL)
#undef XV_TL
  return xv_launch_status();
}

}  // namespace

extern "C" int xv_tuple_capacity(int num_classes, int num_experts) {
  return tuple_count(num_classes, num_experts) > 0 ? 1 : 0;
}

extern "C" int xv_fused_head_multi_tuple_hist_fwd(const float* const* S, const float* const* bias, int num_experts, int n,
                                                  int hi, int wi, int num_classes, const int32_t* group, int num_groups,
                                                  int64_t* hist, int max_workgroups, void* stream) {
  XV_CHECK_ARG(hist && ((uintptr_t)hist & 7) == 0 && xv_group_ok(group, num_groups) && max_workgroups >= 0);
  HeadPtrs ptrs;
  const int rc = tuple_check_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs);
  if (rc != XV_OK) return rc;
  return tuple_launch<false>(ptrs, num_experts, n, hi, wi, num_classes, nullptr, nullptr, group, num_groups, hist,
                             max_workgroups, (hipStream_t)stream);
}

extern "C" int xv_fused_head_multi_lut_count_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi,
                                                 int wi, int num_classes, const uint8_t* lut, const int32_t* labels,
                                                 const int32_t* group, int num_groups, int64_t* cm, int max_workgroups,
                                                 void* stream) {
  XV_CHECK_ARG(lut && labels && cm && ((uintptr_t)lut & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)cm & 7) == 0);
  XV_CHECK_ARG(xv_group_ok(group, num_groups) && max_workgroups >= 0);
  HeadPtrs ptrs;
  const int rc = tuple_check_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs);
  if (rc != XV_OK) return rc;
  return tuple_launch<true>(ptrs, num_experts, n, hi, wi, num_classes, lut, labels, group, num_groups, cm, max_workgroups,
                            (hipStream_t)stream);
}

extern "C" int xv_fused_head_multi_lut_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi,
                                           int wi, int num_classes, const uint8_t* lut, int64_t* fused_label, void* stream) {
  XV_CHECK_ARG(lut && fused_label && ((uintptr_t)lut & 3) == 0 && ((uintptr_t)fused_label & 15) == 0);
  HeadPtrs ptrs;
  const int rc = tuple_check_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs);
  if (rc != XV_OK) return rc;
  const int T = (int)tuple_count(num_classes, num_experts);
  const int64_t nquads = (int64_t)n * hi * wi * 16;  // (8 wi is a multiple of the four pixels of a thread)
  // a workgroup stages the table once: as many workgroups as the quads need, at most eight per CU
  const int64_t need = (nquads + 255) / 256, cap = (int64_t)xv_num_cus() * 8;
  const unsigned grid = (unsigned)(need < cap ? need : cap);
  const size_t lds = (size_t)(T + 15) / 16 * 16;
  hipStream_t s = (hipStream_t)stream;
#define XV_TL(CMV)                                                                                                       \
  hipLaunchKernelGGL((fused_head_multi_lut_kernel<CMV>), dim3(grid), dim3(256), lds, s, ptrs, num_experts, n, hi, wi,    \
                     num_classes, T, lut, fused_label)
  XV_CM_SWITCH(num_classes, XV_TL)
#undef XV_TL
  return xv_launch_status();
}
