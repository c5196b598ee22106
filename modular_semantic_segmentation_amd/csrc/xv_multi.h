// Host half of the heads over two to four experts' low-resolution scores (heads.hip: fused_head_multi, multi_count.hip,
// agreement.hip, calibration.hip, tuple_lut.hip) and of the grouped counting kernels (grouped_score.hip): the argument checks
// and the launch plan every one of their entry points runs, each written once.  Host code only -- what the kernels share is
// in xv_heads.h and xv_fuse.h, and why that stops where it does is told there.
//
// An entry point runs its XV_EINVAL checks first (its own, xv_group_ok, xv_mode_tables_ok), then xv_multi_experts, whose last
// check is the first XV_ESHAPE one: where a call breaks an argument rule and a shape rule, XV_EINVAL wins.  Nothing here
// calls into HIP except xv_grid_bound (the CU count), which comes after all of that.
#pragma once

#include "xv_heads.h"

#define XV_CHECK_OK(call)            \
  do {                               \
    const int rc_ = (call);          \
    if (rc_ != XV_OK) return rc_;    \
  } while (0)

// Launchers of kernels templated on the fusion mode (0 = Bayes, 1 = Dirichlet, 2 = mean; checked before): CALL(args..., MODE),
// beside XV_CM_SWITCH, whose callback passes the padded class count on as an argument.  CALL is a statement or a block.
#define XV_MODE_SWITCH(MODE_, CALL, ...) \
  {                                      \
    if ((MODE_) == 0) {                  \
      CALL(__VA_ARGS__, 0);              \
    } else if ((MODE_) == 1) {           \
      CALL(__VA_ARGS__, 1);              \
    } else {                             \
      CALL(__VA_ARGS__, 2);              \
    }                                    \
  }

// dst[e] = src[e] for the `num` pointers given, each non-null and aligned to align_mask + 1 bytes; unused slots repeat
// expert 0 (never read, never null).  `src` itself is the caller's to check.
template <typename T>
static inline bool xv_fill_expert_slots(const T* const* src, int num, uintptr_t align_mask, const T* (&dst)[XV_MULTI_MAXE]) {
  for (int e = 0; e < XV_MULTI_MAXE; ++e) {
    const T* p = src[e < num ? e : 0];
    if (p == nullptr || ((uintptr_t)p & align_mask) != 0) return false;
    dst[e] = p;
  }
  return true;
}

static inline bool xv_experts_classes_ok(int num_experts, int num_classes) {
  return num_experts >= 2 && num_experts <= XV_MULTI_MAXE && num_classes >= 2 && num_classes <= 32;
}

// The experts of a head: two to four, 2..32 classes, positive sizes, every S[e] 16-byte aligned (the tap loads) and every
// bias[e] 4-byte aligned -> ptrs.  XV_ESHAPE for a map the library cannot address, after every XV_EINVAL of this function.
static inline int xv_multi_experts(const float* const* S, const float* const* bias, int num_experts, int n, int hi, int wi,
                                   int num_classes, HeadPtrs& ptrs) {
  XV_CHECK_ARG(S && bias && xv_experts_classes_ok(num_experts, num_classes) && n > 0 && hi > 0 && wi > 0);
  XV_CHECK_ARG(xv_fill_expert_slots(S, num_experts, 15, ptrs.s) && xv_fill_expert_slots(bias, num_experts, 3, ptrs.b));
  XV_CHECK_SHAPE(xv_dims_sane(n, hi, wi));
  return XV_OK;
}

// mode 0 = Bayes (tab, logprior), 1 = Dirichlet (tab, lognorm, logprior), 2 = mean (no tables): the tables the mode needs, 4-byte aligned
static inline bool xv_mode_tables_ok(int mode, const float* tab, const float* lognorm, const float* logprior) {
  if (mode < 0 || mode > 2) return false;
  if (mode != 2 && !(tab && logprior && ((uintptr_t)tab & 3) == 0 && ((uintptr_t)logprior & 3) == 0)) return false;
  return mode != 1 || (lognorm && ((uintptr_t)lognorm & 3) == 0);
}

// floats of the staged fusion tables of one parameter set: Bayes tab [E][C][CM] + logprior [CM]; Dirichlet tab [E][CM][CM] +
// lognorm [E][CM] + logprior [CM]; the mean none
static inline size_t xv_multi_table_floats(int mode, int num_experts, int num_classes) {
  const size_t c = (size_t)num_classes, cm = (c + 3) / 4 * 4, e = (size_t)num_experts;
  return mode == 0 ? e * c * cm + cm : (mode == 1 ? e * cm * cm + e * cm + cm : 0);
}

// group ids int32 [n] on the device, or none and one group
static inline bool xv_group_ok(const int32_t* group, int num_groups) {
  return ((uintptr_t)group & 3) == 0 && num_groups >= 1 && (group != nullptr || num_groups == 1);
}

// Workgroups a bounded grid may have: per_cu per CU, at most `ceiling` where one is given (> 0: 512 for kernels that end in
// atomics on few addresses, docs/HISTORY.md), at most the caller's max_workgroups where that is given (> 0)
static inline int xv_grid_bound(int per_cu, int ceiling, int max_workgroups) {
  int bound = xv_num_cus() * per_cu;
  if (ceiling > 0 && bound > ceiling) bound = ceiling;
  if (max_workgroups > 0 && max_workgroups < bound) bound = max_workgroups;
  return bound;
}

// How the counting kernels deal their work out: (image, part) slots.  A workgroup counts ONE image at a time into 32-bit
// counters in its LDS and flushes them into that image's group with one 64-bit global atomic per non-zero cell; part p of an
// image takes the steps p, p + parts, ... of its items, `per_step` items a step.  An image is cut into as many parts as its
// steps need, at most its share of the `bound` workgroups, at least one; the grid is the slots, at most the bound: while
// images x parts fit it a workgroup has one slot and flushes once, beyond it a workgroup walks its slots one after the other.
// `counted` is what one image can add to a counter (its pixels): XV_ESHAPE where a part's share of it could pass 32 bits.
struct XvSlotPlan {
  int parts, grid;
};
static inline int xv_slot_plan(int64_t items, int per_step, int64_t counted, int n, int bound, XvSlotPlan& plan) {
  const int64_t need = (items + per_step - 1) / per_step, room = bound / n > 1 ? bound / n : 1;
  plan.parts = (int)(need < room ? need : room);
  XV_CHECK_SHAPE(counted / plan.parts < ((int64_t)1 << 31));
  const int64_t slots = (int64_t)n * plan.parts;
  plan.grid = (int)(slots < bound ? slots : bound);
  return XV_OK;
}
