// conv1_1 of the FCN for gfx950, fp32 image in, bf16 / e4m3 padded-NHWC out: the FMA kernel and the matrix-core kernel
// (the only file built with -mllvm -amdgpu-mfma-vgpr-form, see the Makefile).

#include "xv_common.h"

#pragma clang fp contract(on)  // by the source expression only, as in heads.hip

namespace {

// ---- conv1_1: relu(conv3x3(x) + b) on the raw fp32 input, fp32 math, bf16 padded-NHWC out -------
// simple_fcn.py:39.  One thread = TWO horizontally adjacent pixels x 64 output channels.  The
// 9*CIN x 64 fp32 weight matrix is read through wave-uniform addresses (scalar loads into SGPRs), each
// weight feeding both pixels; results go through LDS so that every store instruction writes whole
// 128-byte pixel rows.
template <int CIN>
__global__ __launch_bounds__(256) void conv_first_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b, __bf16* __restrict__ y, int N,
                                                        int H, int W, int relu) {
  const int Wh = W >> 1;  // pixel pairs per row (W is even: multiple of 16)
  const int npair = N * H * Wh;  // < 2^31, checked by the host
  int pr = blockIdx.x * 256 + threadIdx.x;
  pr = pr < npair ? pr : npair - 1;  // tail lanes recompute the last pair; only in-range pixels are stored
  const int row = pr / Wh;         // n * H + py
  const int px = (pr - row * Wh) * 2;
  const int n = row / H;
  const int py = row - n * H;
  float in[3][4][CIN];  // rows py-1..py+1, columns px-1..px+2
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) {
      const int yy = py + dy - 1, xx = px + dx - 1;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      const float* src = x + (((int64_t)n * H + (ok ? yy : 0)) * W + (ok ? xx : 0)) * CIN;
#pragma unroll
      for (int c = 0; c < CIN; ++c) in[dy][dx][c] = ok ? src[c] : 0.f;
    }
  __shared__ __attribute__((aligned(16))) u32x4 stage[512 * 8];  // [pixel within block][8 slots of 8 channels]
  u32x4* mine = stage + threadIdx.x * 16;
#pragma unroll
  for (int g = 0; g < 4; ++g) {  // 16 output channels at a time (accumulators in VGPRs, weights in SGPRs)
    float a0[16], a1[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) a0[c] = a1[c] = b[g * 16 + c];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
          const int t = (dy * 3 + dx) * CIN + ci;
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            const float wv = w[t * 64 + g * 16 + c];
            a0[c] = fmaf(in[dy][dx][ci], wv, a0[c]);
            a1[c] = fmaf(in[dy][dx + 1][ci], wv, a1[c]);
          }
        }
    if (relu) {
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        a0[c] = fmaxf(a0[c], 0.f);
        a1[c] = fmaxf(a1[c], 0.f);
      }
    }
    // 16-byte slot swizzle (slot ^ pixel) keeps the LDS writes of consecutive lanes on distinct banks
    const int p0 = 2 * threadIdx.x, p1 = p0 + 1;
    mine[(2 * g) ^ (p0 & 7)] = u32x4{pack_bf16x2(a0[0], a0[1]), pack_bf16x2(a0[2], a0[3]), pack_bf16x2(a0[4], a0[5]),
                                     pack_bf16x2(a0[6], a0[7])};
    mine[(2 * g + 1) ^ (p0 & 7)] = u32x4{pack_bf16x2(a0[8], a0[9]), pack_bf16x2(a0[10], a0[11]),
                                         pack_bf16x2(a0[12], a0[13]), pack_bf16x2(a0[14], a0[15])};
    mine[8 + ((2 * g) ^ (p1 & 7))] = u32x4{pack_bf16x2(a1[0], a1[1]), pack_bf16x2(a1[2], a1[3]),
                                           pack_bf16x2(a1[4], a1[5]), pack_bf16x2(a1[6], a1[7])};
    mine[8 + ((2 * g + 1) ^ (p1 & 7))] = u32x4{pack_bf16x2(a1[8], a1[9]), pack_bf16x2(a1[10], a1[11]),
                                               pack_bf16x2(a1[12], a1[13]), pack_bf16x2(a1[14], a1[15])};
  }
  // each wave stores its own 128 pixels: no block barrier needed (the wave's LDS region is private)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int lane = threadIdx.x & 63;
  const int wbase = (threadIdx.x & ~63) * 2;  // first pixel (within the block) of this wave
  const int slot = lane & 7;
  // this lane stores pixel lp = it*8 + (lane>>3) of the wave: pair index advances by 4 per iteration
  int gpair = blockIdx.x * 256 + ((wbase + (lane >> 3)) >> 1);
  int qrow = gpair / Wh;  // n * H + y
  int qxh = gpair - qrow * Wh;
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int lp = it * 8 + (lane >> 3);
    if (gpair < npair) {
      const int qn = qrow / H;
      const int qy = qrow - qn * H;
      const u32x4 v = stage[(wbase + lp) * 8 + (slot ^ (lp & 7))];
      *reinterpret_cast<u32x4*>(y + (((int64_t)qn * (H + 2) + (qy + 1)) * (W + 2) + (qxh * 2 + (lp & 1) + 1)) * 64 +
                                slot * 8) = v;
    }
    gpair += 4;
    qxh += 4;
    if (qxh >= Wh) {  // Wh >= 8: at most one row wrap per step
      qxh -= Wh;
      qrow += 1;
    }
  }
}

// ---- conv1_1 on the matrix cores -------------------------------------------------------------------------------------
// The same layer (fp32 image, fp32 weights, fp32 accumulation, one bf16 rounding at the end) as 16 x 16 x 32 bf16 MFMAs:
// every fp32 operand is split EXACTLY into three bf16 terms (x = xh + xm + xl: 3 x 8 significant bits), and the six
// products down to 2^-16 relative (h.h, h.m, m.h, m.m, h.l, l.h) are accumulated in fp32, smallest first -- the dropped
// terms are below 2^-24 of |x||w|, i.e. below the fp32 rounding of the plain FMA chain.  K = 9 CIN <= 27 fits one
// MFMA: k-group g (8 values, lanes 16 g .. 16 g + 15) holds image row dy = g, columns dx = 0..2 x CIN channels in
// memory order (8 of its 9 values for CIN = 3); the three leftover values (dx = 2, ci = 2 of each row) form k-group 3.
// One wave = one tile of 16 consecutive pixels of an image row x 64 channels: 24 MFMAs against 1,728 packed FMAs per
// lane pair of conv_first_kernel, which leaves the layer bound by its output stores.  The tile goes through a 2 KB LDS
// transpose so that each store instruction writes eight whole 128-byte pixel rows (1 KB contiguous).
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {  // one v_cvt_pk_bf16_f32
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}

// OUT8: the map is written as e4m3 of value * out_mul (the fp8 graph where conv1_2 takes e4m3 operands, fcn.fp8_plan): a
// tile is then ONE contiguous 1 KB store (16 pixels x 64 channels)
// G7: the map is not written at all; every pixel goes straight to its places in the operand of AdapNet's 7x7 stride-2 conv
// (xv_gather_conv7s2's z [N,H/2,W/2,9*64], adapnet.py:126-127): row variant 0 / 1 of an even row Y at j = Y/2 / Y/2 - 1,
// variant 2 of an odd row at j = (Y-1)/2, columns alike -- 2.25 stores of 128 bytes per pixel on average instead of one,
// and neither the 0.6 GB map nor the gather's read of it.  Positions of z without a source pixel (variant 1 in the last
// row / column) are never written: the caller's buffer holds zeros there (as xv_gather_conv7s2 leaves them).
template <int CIN, bool OUT8 = false, bool G7 = false>
__global__ __launch_bounds__(256) void conv_first_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ b, __bf16* __restrict__ y, int N,
                                                             int H, int W, int relu, int tpw, float out_mul = 1.f) {
  static_assert(!(OUT8 && G7), "the gathered form writes bf16");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int Wt = W >> 4;  // tiles per image row (W is a multiple of 16, checked by the host)
  const int ntiles = N * H * Wt;
  __shared__ __attribute__((aligned(16))) u32x4 stage_all[4 * 128];
  u32x4* stage = stage_all + wave * 128;  // [16 pixels][8 slots of 8 channels], private to the wave

  // weight fragments (A operand: row = channel j of the 16-channel block, k-group g), split three ways.  The bias
  // rides in the first spare k slot of group 3 against a constant 1.0 on the image side (1.0 = xh exactly, so the
  // three terms wh + wm + wl = b enter the sum exactly): the accumulators start from zero and cost no registers.
  constexpr int BIAS_E = CIN == 3 ? 3 : 0;
  bf16x8 wh[4], wm[4], wl[4];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    float wv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int dy, dx, ci;
      const bool ok = first_k_map<CIN>(g, e, dy, dx, ci);
      wv[e] = ok ? w[((dy * 3 + dx) * CIN + ci) * 64 + jb * 16 + j] : 0.f;
      if (e == BIAS_E) wv[e] = g == 3 ? b[jb * 16 + j] : wv[e];
    }
    split3_bf16x8(wv, wh[jb], wm[jb], wl[jb]);
  }

  // Lane constants of the tap loads.  A lane of k-group g < 3 reads image row py + g - 1 at columns px - 1, px, px + 1
  // (CIN contiguous floats each); a lane of k-group 3 reads column px + 1 of rows py - 1, py, py + 1 (CIN == 3 only: it
  // uses the last channel).  Position t is at float offset (tile origin) + lc + t * lstride; it lies outside the image
  // when one of the tile's edge flags (bit 0 top row, 1 bottom row, 2 first tile of the row, 3 last tile; bit 4: set
  // always, kills the lanes that never load; bit 5: there is no such tile, kills every lane) meets the position's
  // kill mask.
  const bool main = g < 3;
  const int lc = main ? ((g - 1) * W + j - 1) * CIN : (-W + j + 1) * CIN;
  const int lstride = main ? CIN : W * CIN;
  int kill[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int dy = main ? g : t, dx = main ? t : 2;
    kill[t] = 32 | (dy == 0 ? 1 : 0) | (dy == 2 ? 2 : 0) | ((j == 0 && dx == 0) ? 4 : 0) | ((j == 15 && dx == 2) ? 8 : 0) |
              ((CIN == 1 && !main) ? 16 : 0);
  }
  const int slot = ((g & 1) << 1) | (g >> 1);
  const int st_w0 = j * 8 + (slot ^ (j & 7)), st_w1 = j * 8 + ((slot + 4) ^ (j & 7));
  const int pj0 = lane >> 3, sl = lane & 7;
  const int st_r0 = pj0 * 8 + (sl ^ (pj0 & 7)), st_r1 = (pj0 + 8) * 8 + (sl ^ (pj0 & 7));
  const int st_g = pj0 * 64 + sl * 8;

  // wave-uniform tile walk (no divisions in the loop): tile -> (image n, row py, tile tx of the row)
  // a wave takes a contiguous run of tpw tiles (its stores and taps stream through memory; measured 5-10 % ahead of a
  // grid-stride assignment); tpw = 0: grid stride
  const int wstride = tpw ? 1 : gridDim.x * 4;
  int tile = tpw ? (blockIdx.x * 4 + wave) * tpw : blockIdx.x * 4 + wave;
  const int tile_end = tpw ? (tile + tpw < ntiles ? tile + tpw : ntiles) : ntiles;
  int n, py, tx;
  {
    const int row = tile / Wt;
    tx = tile - row * Wt;
    n = row / H;
    py = row - n * H;
  }
  const int drow = wstride / Wt, dtx = wstride - drow * Wt;
  const int dn = drow / H, dpy = drow - dn * H;

  // requests the taps of tile TILE = (n, py, tx), unmasked: they are masked where they are consumed, one tile later, so
  // that nothing here waits for the loads
#define XV_FIRST_LOAD(TILE)                                                                                           \
  {                                                                                                                   \
    const int sbase = ((n * H + py) * W + tx * 16) * CIN;                                                             \
    const int edge = (py == 0 ? 1 : 0) | (py == H - 1 ? 2 : 0) | (tx == 0 ? 4 : 0) | (tx == Wt - 1 ? 8 : 0) | 16 |    \
                     ((TILE) < tile_end ? 0 : 32);                                                                      \
    _Pragma("unroll") for (int t = 0; t < 3; ++t) {                                                                   \
      ok[t] = (kill[t] & edge) == 0;                                                                                  \
      const int off = ok[t] ? sbase + lc + t * lstride : 0;                                                           \
      _Pragma("unroll") for (int c = 0; c < CIN; ++c) raw[t][c] = x[off + c];                                         \
    }                                                                                                                 \
  }

  const uint32_t floor2 = relu ? 0u : 0x80008000u;  // relu as a packed signed-integer max (xv_common.h); -32768 = none
  float raw[3][CIN];
  bool ok[3];
  XV_FIRST_LOAD(tile)
  for (; tile < tile_end; tile += wstride) {
    // B operand of this tile (column = pixel j, k-group g): masked taps in k order, split three ways
    float v[8];
    if (CIN == 3) {
      v[0] = ok[0] ? (main ? raw[0][0] : raw[0][2]) : 0.f;
      v[1] = main ? (ok[0] ? raw[0][1] : 0.f) : (ok[1] ? raw[1][2] : 0.f);
      v[2] = main ? (ok[0] ? raw[0][2] : 0.f) : (ok[2] ? raw[2][2] : 0.f);
      v[3] = main ? (ok[1] ? raw[1][0] : 0.f) : 1.f;  // k-group 3: the bias slot
      v[4] = main && ok[1] ? raw[1][1] : 0.f;
      v[5] = main && ok[1] ? raw[1][2] : 0.f;
      v[6] = main && ok[2] ? raw[2][0] : 0.f;
      v[7] = main && ok[2] ? raw[2][1] : 0.f;
    } else {
      v[0] = main ? (ok[0] ? raw[0][0] : 0.f) : 1.f;  // k-group 3: the bias slot
      v[1] = ok[1] ? raw[1][0] : 0.f, v[2] = ok[2] ? raw[2][0] : 0.f;
      v[3] = v[4] = v[5] = v[6] = v[7] = 0.f;
    }
    bf16x8 xh, xm, xl;
    split3_bf16x8(v, xh, xm, xl);
    __bf16* dst = y + (((int64_t)n * (H + 2) + (py + 1)) * (W + 2) + (tx * 16 + 1)) * 64 + st_g;
    char* dst8 = reinterpret_cast<char*>(y) + (((int64_t)n * (H + 2) + (py + 1)) * (W + 2) + (tx * 16 + 1)) * 64 + lane * 16;
    // G7: the lane's pixel X = 16 tx + pj0 (and X + 8: four operand columns further) in row variant A = 0 (even py) / 2 (odd)
    // and column variant C = 0 (even X) / 2 (odd), at operand pixel (py >> 1, X >> 1)
    char* zA_C = nullptr;
    bool g7_d0 = false, g7_rowb = false;
    if constexpr (G7) {
      const int Ho = H >> 1, Wo = W >> 1, X = tx * 16 + pj0;
      const int rvA = (py & 1) ? 2 : 0, cvC = (pj0 & 1) ? 2 : 0;
      zA_C = reinterpret_cast<char*>(y) + ((((int64_t)n * (Ho + 2) + (py >> 1) + 1) * (Wo + 2) + (X >> 1) + 1) * 576 + (rvA * 3 + cvC) * 64) * 2 + sl * 16;
      g7_d0 = X >= 2;                        // the even pixel's second column place (variant 1 at X/2 - 1) exists
      g7_rowb = (py & 1) == 0 && py >= 2;    // the even row's second place (variant 1 at py/2 - 1) exists
    }
    // next tile: advance the walk and request its taps; they land behind this tile's MFMAs, and this tile's stores are
    // issued after them (the vector-memory counter retires in order: waiting for the taps then never waits for the
    // stores issued behind them)
    {
      tx += dtx;
      const int c1 = tx >= Wt ? 1 : 0;
      tx -= c1 ? Wt : 0;
      py += dpy + c1;
      const int c2 = py >= H ? 1 : 0;
      py -= c2 ? H : 0;
      n += dn + c2;
    }
    XV_FIRST_LOAD(tile + wstride)
    __builtin_amdgcn_sched_barrier(0x78f);  // no memory request may sink below the MFMAs (everything else may move)
    f32x4 acc[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[jb], xl, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[jb], xh, acc[jb], 0, 0, 0);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm[jb], xm, acc[jb], 0, 0, 0);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[jb], xm, acc[jb], 0, 0, 0);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm[jb], xh, acc[jb], 0, 0, 0);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) acc[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[jb], xh, acc[jb], 0, 0, 0);
    if constexpr (OUT8) {
      // lane (pixel j, row group g) holds channels 16 jb + 4 g .. + 3 of block jb: one dword of e4m3 each, at 16-byte slot
      // jb ^ ((j >> 1) & 3) of the pixel's 64-byte row in the wave's stage (two-way write conflicts: free); read back as
      // 16 bytes per lane = pixel lane >> 2, slot lane & 3
      uint32_t* st32 = reinterpret_cast<uint32_t*>(stage);
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        f32x4 t = acc[jb];
        if (relu) t = f32x4{fmaxf(t.x, 0.f), fmaxf(t.y, 0.f), fmaxf(t.z, 0.f), fmaxf(t.w, 0.f)};
        st32[j * 16 + ((jb ^ ((j >> 1) & 3)) << 2) + g] = xv_pack_fp8x4(t.x, t.y, t.z, t.w, out_mul);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int pj = lane >> 2, sl = lane & 3;
      const u32x4 r = stage[pj * 4 + (sl ^ ((pj >> 1) & 3))];
      *reinterpret_cast<u32x4*>(dst8) = r;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    u32x2 packed[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
      packed[jb] = u32x2{pk_max_i16(cvt_pk_bf16(acc[jb][0], acc[jb][1]), floor2),
                         pk_max_i16(cvt_pk_bf16(acc[jb][2], acc[jb][3]), floor2)};
    // lane (pixel j, row group g) now holds 8 consecutive channels of each 32-channel pair, starting at channel
    // {0, 16, 8, 24}[g] of the pair: 16-byte slot {0, 2, 1, 3}[g] + 4 pair of the pixel's 128-byte row
    u32x4 o0, o1;
    xv_pair16(packed[0], packed[1], o0);
    xv_pair16(packed[2], packed[3], o1);
    stage[st_w0] = o0;
    stage[st_w1] = o1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const u32x4 r0 = stage[st_r0], r1 = stage[st_r1];
    if constexpr (G7) {
      const int Wo = W >> 1;
      const int64_t rowb = -(int64_t)(Wo + 2) * 1152 + 3 * 128;   // row variant 0 -> 1, one operand row up
      const bool even_x = (pj0 & 1) == 0;
      *reinterpret_cast<u32x4*>(zA_C) = r0;
      *reinterpret_cast<u32x4*>(zA_C + 4 * 1152) = r1;
      if (even_x) {                                                // column variant 0 -> 1, one operand column to the left
        if (g7_d0) *reinterpret_cast<u32x4*>(zA_C - 1152 + 128) = r0;
        *reinterpret_cast<u32x4*>(zA_C + 3 * 1152 + 128) = r1;
      }
      if (g7_rowb) {
        *reinterpret_cast<u32x4*>(zA_C + rowb) = r0;
        *reinterpret_cast<u32x4*>(zA_C + rowb + 4 * 1152) = r1;
        if (even_x) {
          if (g7_d0) *reinterpret_cast<u32x4*>(zA_C + rowb - 1152 + 128) = r0;
          *reinterpret_cast<u32x4*>(zA_C + rowb + 3 * 1152 + 128) = r1;
        }
      }
    } else {
      *reinterpret_cast<u32x4*>(dst) = r0;
      *reinterpret_cast<u32x4*>(dst + 8 * 64) = r1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
#undef XV_FIRST_LOAD
}

}  // namespace

// block_0_1 + the gather of block_0_2 in one pass (conv_first_mfma_kernel<CIN, false, true>): z as xv_gather_conv7s2 writes it.
extern "C" int xv_conv2d_first_gather7s2_fwd(const float* x, int n, int h, int w, int cin, const float* w_hwio,
                                             const float* bias, const xv_act* z, int relu, void* stream) {
  XV_CHECK_ARG(x && w_hwio && bias && z && z->data);
  XV_CHECK_ARG(z->dtype == XV_BF16);
  XV_CHECK_SHAPE(n > 0 && h > 0 && w >= 16 && (cin == 1 || cin == 3) && (w & 15) == 0 && (h & 1) == 0 &&
                 (int64_t)n * h * w * cin < 0x7ff00000);
  XV_CHECK_SHAPE(z->n == n && z->h == h / 2 && z->w == w / 2 && z->c == 576);
  const int64_t ntiles = (int64_t)n * h * (w / 16);
  const int64_t want = (ntiles + 3) / 4, cap = (int64_t)xv_num_cus() * 4;  // four workgroups per CU, as xv_conv2d_first_fwd
  const int64_t g0 = want < cap ? want : cap;
  const int tpw = (int)((ntiles + g0 * 4 - 1) / (g0 * 4));
  const unsigned g2 = (unsigned)((ntiles + (int64_t)tpw * 4 - 1) / ((int64_t)tpw * 4));
  hipStream_t s = (hipStream_t)stream;
  if (cin == 1)
    hipLaunchKernelGGL((conv_first_mfma_kernel<1, false, true>), dim3(g2), dim3(256), 0, s, x, w_hwio, bias, (__bf16*)z->data, n, h,
                       w, relu, tpw, 1.f);
  else
    hipLaunchKernelGGL((conv_first_mfma_kernel<3, false, true>), dim3(g2), dim3(256), 0, s, x, w_hwio, bias, (__bf16*)z->data, n, h,
                       w, relu, tpw, 1.f);
  return xv_launch_status();
}

extern "C" int xv_conv2d_first_fwd(const float* x, int n, int h, int w, int cin, const float* w_hwio,
                                   const float* bias, const xv_act* y, int relu, void* stream) {
  XV_CHECK_ARG(x && w_hwio && bias && y && y->data);
  XV_CHECK_ARG(y->dtype == XV_BF16 || y->dtype == XV_FP8);
  XV_CHECK_SHAPE(n > 0 && h > 0 && w > 0 && cin >= 1 && cin <= 4);
  XV_CHECK_SHAPE(y->n == n && y->h == h && y->w == w && y->c == 64);
  const bool out8 = y->dtype == XV_FP8;  // e4m3 output: the matrix-core kernel only (1 / 3 channels, w % 16 == 0)
  if (out8) XV_CHECK_SHAPE((cin == 1 || cin == 3) && (w & 15) == 0 && y->scale_exp > -100 && y->scale_exp < 100);
  const float out_mul = out8 ? exp2f((float)-y->scale_exp) : 1.f;
  XV_CHECK_SHAPE((w & 1) == 0 && w >= 16 && (int64_t)n * h * (w / 2) < 0x7fffff00);
  const int64_t npair = (int64_t)n * h * (w / 2);
  const unsigned grid = (unsigned)((npair + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  __bf16* yp = (__bf16*)y->data;
  // The MFMA form takes whole 16-pixel tiles and 32-bit float offsets into x; every other shape keeps the FMA kernel.
  if ((cin == 1 || cin == 3) && (w & 15) == 0 && (int64_t)n * h * w * cin < 0x7ff00000) {
    // 98 VGPRs: five workgroups resident per CU; measured at 8 x 384 x 768 with grid-stride tiles: 5 per CU (one round)
    // 78 / 102 us (depth / RGB), 8: 70 / 92, 16: 65 / 92, 32: 67 / 98, 64: 83 / 122; with contiguous runs per wave 8 per CU:
    // 59 / 84, 16: 62 / 96, 32: 71 / 101; 4 or 5 per CU (all resident, one round): 57 / 83; 3: 88 / 100; 6 (one more than
    // fits): 71 / 97.  4: still one round if a rebuild needs a few more registers
    const int64_t ntiles = (int64_t)n * h * (w / 16);
    const int64_t want = (ntiles + 3) / 4, cap = (int64_t)xv_num_cus() * 4;
    const int64_t g0 = want < cap ? want : cap;
    const int tpw = (int)((ntiles + g0 * 4 - 1) / (g0 * 4));               // tiles per wave
    const unsigned g2 = (unsigned)((ntiles + (int64_t)tpw * 4 - 1) / ((int64_t)tpw * 4));
    if (out8) {
      if (cin == 1)
        hipLaunchKernelGGL((conv_first_mfma_kernel<1, true>), dim3(g2), dim3(256), 0, s, x, w_hwio, bias, yp, n, h, w, relu, tpw,
                           out_mul);
      else
        hipLaunchKernelGGL((conv_first_mfma_kernel<3, true>), dim3(g2), dim3(256), 0, s, x, w_hwio, bias, yp, n, h, w, relu, tpw,
                           out_mul);
    } else if (cin == 1)
      hipLaunchKernelGGL(conv_first_mfma_kernel<1>, dim3(g2), dim3(256), 0, s, x, w_hwio, bias, yp, n, h, w, relu, tpw, 1.f);
    else
      hipLaunchKernelGGL(conv_first_mfma_kernel<3>, dim3(g2), dim3(256), 0, s, x, w_hwio, bias, yp, n, h, w, relu, tpw, 1.f);
    return xv_launch_status();
  }
  if (out8) return XV_ESHAPE;
  switch (cin) {
    case 1: hipLaunchKernelGGL(conv_first_kernel<1>, dim3(grid), dim3(256), 0, s, x, w_hwio, bias, yp, n, h, w, relu); break;
    case 2: hipLaunchKernelGGL(conv_first_kernel<2>, dim3(grid), dim3(256), 0, s, x, w_hwio, bias, yp, n, h, w, relu); break;
    case 3: hipLaunchKernelGGL(conv_first_kernel<3>, dim3(grid), dim3(256), 0, s, x, w_hwio, bias, yp, n, h, w, relu); break;
    default: hipLaunchKernelGGL(conv_first_kernel<4>, dim3(grid), dim3(256), 0, s, x, w_hwio, bias, yp, n, h, w, relu); break;
  }
  return xv_launch_status();
}
