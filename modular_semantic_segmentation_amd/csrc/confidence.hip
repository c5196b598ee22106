// Confidence maps for gfx950: the fused label with its calibrated confidence per pixel -- what the reliability tables of
// calibration.hip count, handed out instead of counted.
//
// THE MAP.  Class scores s[k], k < C, in the log domain, as calibration.hip takes them: the fused score of xv_bayes_fuse /
// xv_dirichlet_fuse, for the mean ln(1e-20 + mean_e p_e[k]), for one expert its logits.  `win` is the first maximum -- the
// label the existing route writes; a temperature never moves it -- and at the temperature T > 0 (xv_conf.h: conf_pixel, the
// ONE place the arithmetic is written, on the statements of calib_pixel)
//   conf = 1 / sum_k exp((s[k] - s[win]) / T), entropy of that softmax in nats, margin = conf - the second largest probability
//   label = conf < threshold ? void_label : win
// (uint32)(conf 2^24) of a written confidence is the q the calibration kernels count, integer for integer.
//
//   xv_confidence_map                     from a materialised map of scores or probabilities
//   xv_fused_head_multi_confidence_fwd    from the experts' low-resolution scores: the statements of
//                                         fused_head_multi_calibration_kernel (calibration.hip) up to the fused scores and
//                                         `win`, then conf_pixel and the stores.  No LDS counters, no labels input, no
//                                         probability or score map
//
// Each of the four outputs may be null and is then not touched; at least one is given.  A thread takes ONE pixel: a wave's
// store is then 64 consecutive int64 (512 bytes) or floats (256 bytes) per output, every one a run of whole cache lines, and
// the fused form keeps the registers of the calibration kernel of the same mode without its counting (tests/
// test_confidence_registers_cpu.py pins the waves).  The grid is bounded (xv_multi.h: xv_grid_bound, eight 256-thread
// workgroups per CU) and strides over the pixels, so a workgroup stages the fusion tables once for all its pixels.
#include "xv_common.h"
#include "xv_heads.h"  // the heads' per-pixel pieces and, through it, xv_fuse.h (sets `fp contract(on)` for what follows)
#include "xv_conf.h"
#include "xv_multi.h"  // the host side: argument checks and the grid bound

namespace {

constexpr int XV_CONF_THREADS = 256;
constexpr int XV_CONF_PER_CU = 8;

// what a launch writes and how: the temperature, the threshold and the four outputs, each of which may be null
struct ConfOut {
  float temperature, threshold;
  int64_t void_label;
  int64_t* label;
  float* conf;
  float* entropy;
  float* margin;
};

// one pixel's scores and winner -> its entries of the maps that are asked for
template <int CM>
__device__ static __forceinline__ void conf_store(const float (&v)[CM], int C, int win, int64_t at, const ConfOut& out) {
  float conf, entropy, margin;
  conf_pixel<CM>(v, C, win, calib_pick<CM>(v, win), out.temperature, conf, entropy, margin);
  if (out.label != nullptr) out.label[at] = conf_label(win, conf, out.threshold, out.void_label);
  if (out.conf != nullptr) out.conf[at] = conf;
  if (out.entropy != nullptr) out.entropy[at] = entropy;
  if (out.margin != nullptr) out.margin[at] = margin;
}

// waves per SIMD the Dirichlet forms are held to: what the calibration kernel of the same class count reaches under its
// 512-thread bound.  Left alone the compiler keeps table rows of the rolled expert loop in registers (12 classes: 174
// registers, two waves; 16 classes: 322, one), as it does in fused_head_multi_kernel (heads.hip: xv_multi_waves).
constexpr int xv_conf_waves(int cm, int mode) { return mode != 1 ? 1 : (cm <= 20 ? 4 : (cm <= 28 ? 3 : 2)); }

// ---- from the experts' low-resolution scores: the statements of fused_head_multi_calibration_kernel up to v and win -------
template <int CM, int MODE>
__global__ __launch_bounds__(XV_CONF_THREADS) __attribute__((amdgpu_waves_per_eu(xv_conf_waves(CM, MODE)))) void fused_head_multi_confidence_kernel(
    HeadPtrs ptrs, int E, int N, int Hi, int Wi, int C, const float* __restrict__ tab_g, const float* __restrict__ lognorm_g,
    const float* __restrict__ logprior_g, ConfOut out) {
  extern __shared__ __attribute__((aligned(16))) float conf_tab[];
  const int rows = MODE == 1 ? CM : C;  // table rows per expert
  float* ln = conf_tab + E * rows * CM;            // [E][CM], Dirichlet only
  float* lp = ln + (MODE == 1 ? E * CM : 0);       // [CM]
  if constexpr (MODE == 0) fuse_stage_rows<CM>(conf_tab, tab_g, E * C, C);
  if constexpr (MODE == 1) fuse_stage_dirichlet<CM>(conf_tab, ln, tab_g, lognorm_g, E, C);
  if constexpr (MODE != 2) {
    fuse_stage_rows<CM>(lp, logprior_g, 1, C);
    __syncthreads();
  }
  const int Ho = Hi * 8, Wo = Wi * 8;
  const int64_t ppi = (int64_t)Ho * Wo;  // pixels of one image
  const int64_t total = (int64_t)N * ppi;
  for (int64_t at = (int64_t)blockIdx.x * XV_CONF_THREADS + threadIdx.x; at < total; at += (int64_t)gridDim.x * XV_CONF_THREADS) {
    const int img = (int)(at / ppi);
    const int64_t pix = at - (int64_t)img * ppi;
    const int ox = (int)(pix % Wo);
    const int oy = (int)(pix / Wo);
    int iy1, ix1;
    float wy1, wy0, wx1, wx0;
    bilinear_taps<8>(oy, iy1, wy1, wy0);
    bilinear_taps<8>(ox, ix1, wx1, wx0);
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
          const f32x2* rowk = reinterpret_cast<const f32x2*>(conf_tab + (e * CM + k) * CM);
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
        const f32x4* row = reinterpret_cast<const f32x4*>(conf_tab + (e * C + le) * CM);
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
    conf_store<CM>(v, C, win, at, out);
  }
}

// ---- from a materialised map: values float [npix][C], scores (kind 0) or probabilities (kind 1) ---------------------------
template <int CM>
__global__ __launch_bounds__(XV_CONF_THREADS) void confidence_map_kernel(const float* __restrict__ values, int kind, int64_t npix,
                                                                         int C, int vec, ConfOut out) {
  for (int64_t at = (int64_t)blockIdx.x * XV_CONF_THREADS + threadIdx.x; at < npix; at += (int64_t)gridDim.x * XV_CONF_THREADS) {
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
    conf_store<CM>(v, C, win, at, out);
  }
}

// a temperature finite and positive, a threshold finite and in [0, 1], at least one output, every given output aligned to its
// element -> out
bool conf_args_ok(float temperature, float threshold, int64_t void_label, int64_t* label_out, float* conf_out,
                  float* entropy_out, float* margin_out, ConfOut& out) {
  if (!(temperature > 0.f) || !(temperature <= 3.4028234663852886e38f)) return false;  // (NaN fails the first test)
  if (!(threshold >= 0.f) || !(threshold <= 1.f)) return false;
  if (label_out == nullptr && conf_out == nullptr && entropy_out == nullptr && margin_out == nullptr) return false;
  if (((uintptr_t)label_out & 7) != 0 || (((uintptr_t)conf_out | (uintptr_t)entropy_out | (uintptr_t)margin_out) & 3) != 0)
    return false;
  out = ConfOut{temperature, threshold, void_label, label_out, conf_out, entropy_out, margin_out};
  return true;
}

// one workgroup per 256 pixels, at most eight per CU
int conf_grid(int64_t npix) {
  const int64_t need = (npix + XV_CONF_THREADS - 1) / XV_CONF_THREADS;
  const int bound = xv_grid_bound(XV_CONF_PER_CU, 0, 0);
  return (int)(need < bound ? need : bound);
}

}  // namespace

extern "C" int xv_confidence_map(const float* values, int kind, int n, int64_t ppi, int num_classes, float temperature,
                                 float threshold, int64_t void_label, int64_t* label_out, float* conf_out, float* entropy_out,
                                 float* margin_out, void* stream) {
  XV_CHECK_ARG(values && ((uintptr_t)values & 3) == 0 && n >= 1 && ppi >= 1 && (kind == 0 || kind == 1));
  XV_CHECK_ARG(num_classes >= 2 && num_classes <= 32);
  ConfOut out;
  XV_CHECK_ARG(conf_args_ok(temperature, threshold, void_label, label_out, conf_out, entropy_out, margin_out, out));
  XV_CHECK_SHAPE(ppi <= ((int64_t)1 << 40) / n);
  const int64_t npix = (int64_t)n * ppi;
  const int grid = conf_grid(npix);
  const int vec = (num_classes & 3) == 0 && ((uintptr_t)values & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
#define XV_CO(CMV) \
  hipLaunchKernelGGL(confidence_map_kernel<CMV>, dim3(grid), dim3(XV_CONF_THREADS), 0, s, values, kind, npix, num_classes, vec, out)
  XV_CM_SWITCH(num_classes, XV_CO)
#undef XV_CO
  return xv_launch_status();
}

extern "C" int xv_fused_head_multi_confidence_fwd(const float* const* S, const float* const* bias, int num_experts, int n, int hi,
                                                  int wi, int num_classes, int mode, const float* tab, const float* lognorm,
                                                  const float* logprior, float temperature, float threshold, int64_t void_label,
                                                  int64_t* label_out, float* conf_out, float* entropy_out, float* margin_out,
                                                  void* stream) {
  XV_CHECK_ARG(xv_mode_tables_ok(mode, tab, lognorm, logprior));
  ConfOut out;
  XV_CHECK_ARG(conf_args_ok(temperature, threshold, void_label, label_out, conf_out, entropy_out, margin_out, out));
  HeadPtrs ptrs;
  XV_CHECK_OK(xv_multi_experts(S, bias, num_experts, n, hi, wi, num_classes, ptrs));
  const int grid = conf_grid((int64_t)n * hi * wi * 64);
  const size_t lds = xv_multi_table_floats(mode, num_experts, num_classes) * 4;  // (17 KB at most: no attribute to raise)
  hipStream_t s = (hipStream_t)stream;
#define XV_CF_MODE(CMV, MODE)                                                                                              \
  hipLaunchKernelGGL((fused_head_multi_confidence_kernel<CMV, MODE>), dim3(grid), dim3(XV_CONF_THREADS), lds, s, ptrs,      \
                     num_experts, n, hi, wi, num_classes, tab, lognorm, logprior, out)
#define XV_CF(CMV) XV_MODE_SWITCH(mode, XV_CF_MODE, CMV)
  XV_CM_SWITCH(num_classes, XV_CF)
#undef XV_CF
#undef XV_CF_MODE
  return xv_launch_status();
}
