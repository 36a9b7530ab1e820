// lconv_i8_core.h — the body of the INT8 layer conv, shared by its two sets of entry points: k_lconv_i8<KW, CIN, COUT, ..>
// with constant widths (lconv_i8.hip) and k_lconv_i8_any<KW, ..> with the widths as launch arguments (lconv_i8_any.hip),
// as layer_kernels.h serves kernels.hip and conv_any.hip.  Device code only: include it from a .hip unit.
//
// k_lconv_i8 runs one conv of a layer-wise block on v_mfma_i32_16x16x64_i8.  Operand layout:
//   activations  int8 [pos][C / 16][361][16]   (the fp16 path's [pos][C / 8][361][8] with 16 channels per 16-byte point)
//   weights      int8 [cout pass][K slice][tap][cout tile][64 lanes][16]  (lconv_i8.h pack_lconv_i8)
// MFMA lane map (checked on the GPU with exact asymmetric integer data): lane l holds A[row l & 15]
// [k = 16 (l >> 4) + j] and B[k = 16 (l >> 4) + j][col l & 15], j = 0..15, and D[row 4 (l >> 4) + r][col l & 15] in
// register r.  A = weights (row = output channel), B = activations (column = board point).
//
// A workgroup of four waves owns one position and one pass of 64 output channels.  Input channels are staged in
// 64-channel slices into a zero-bordered 21 x 21 LDS image (double-buffered: the next slice's global loads are in
// flight while the current one runs).  Wave w takes the 16-point tiles w, w + 4, .. of the 23 that cover the board
// and all four 16-channel output tiles: per tap it reads four weight fragments from global (shared by the workgroup's
// waves through L1) and six activation fragments from LDS, and issues 24 MFMAs.
#pragma once
#include "lconv_i8.h"
#include "conv_core.h"
#include "layer_kernels.h"

namespace p3 {

typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kPad = 21;                       // padded board side
constexpr int kPadPts = kPad * kPad;           // 441
constexpr int kSliceCh = 64;                   // input channels per K slice
constexpr int kSliceBytes = (kSliceCh / 16) * kPadPts * 16;   // 28,224
constexpr int kWgI8 = 256;
constexpr int kStageItems = (kSliceCh / 16) * kNLoc;          // 1,444 sixteen-byte points per slice
constexpr int kStagePerThread = (kStageItems + kWgI8 - 1) / kWgI8; // 6
constexpr int kTiles = (kNLoc + 15) / 16;                      // 23 point tiles
constexpr int kTilesPerWave = (kTiles + 3) / 4;                // 6

__device__ __forceinline__ int pad_index(int loc) { return (loc / 19 + 1) * kPad + loc % 19 + 1; }

// q = clamp(rint(y / s), -127, 127); a zero scale (an all-zero tensor) quantizes everything to 0
__device__ __forceinline__ unsigned q8(float y, float s) {
  if (!(s > 0.0f)) return 0u;
  float q = __builtin_rintf(y / s);
  q = fminf(fmaxf(q, -127.0f), 127.0f);
  return (unsigned)((int)q) & 0xffu;
}

// PRE staging: 16 channels of one point from the raw fp16 stream, mish(bn(.)) and quantized
__device__ __forceinline__ i32x4 stage_pre(const h8& lo, const h8& hi, const float* sc, const float* sh, int c0, float s) {
  i32x4 r;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    unsigned u = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = 4 * w + b, c = c0 + j;
      const float x = (float)(j < 8 ? lo[j] : hi[j - 8]);
      u |= q8(mish_f(x * sc[c] + sh[c]), s) << (8 * b);
    }
    r[w] = (int)u;
  }
  return r;
}

// The body of k_lconv_i8 and k_lconv_i8_any.  WI / WO: the input and output widths as policies (layer_kernels.h FixedW<N>
// or RuntimeW).  They enter through the slice count CIN / 64, the pass count COUT / 64 and the layout strides only: with
// FixedW all three fold to the constants the templated kernel always had, with RuntimeW they are registers.  The LDS
// image (two slices) depends on neither.  One slice (CIN = 64): nothing is prefetched and image 0 alone is read; image
// s & 1 is never read before stage_store(s) and the barrier behind it.
// OUT16 (lconv_conv3.hip, P3HIP_FLAG_INT8_CONV3: the consumer is an fp16 1x1 conv): the activated tensor goes out as fp16
// in the fp16 layout, (_Float16) mish(bn_out(y)), the fp16 plan's own rounding point, and no output scale is read.
template <int KW, class WI, class WO, bool PRE, bool ACT, bool RES, bool DUAL, bool OUT16 = false>
__device__ __forceinline__ void lconv_i8_body(LConvI8Args a, WI wi, WO wo) {
  static_assert(!(ACT && (RES || DUAL)), "act stores the activated tensor only");
  if constexpr (WI::fixed && WO::fixed)
    static_assert(WI::get() % kSliceCh == 0 && WO::get() % 64 == 0, "64-channel slices and passes");
  constexpr int KK = KW * KW;
  const int CIN = wi.get(), COUT = wo.get();
  const int NS = CIN / kSliceCh, NCP = COUT / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cp = blockIdx.x % NCP;
  const int pos = blockIdx.x / NCP;
  if (pos >= a.npos) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4;

  // the border of both images stays zero (only interior points are ever staged)
  for (int i = tid; i < 2 * kSliceBytes / 16; i += kWgI8) *(i32x4*)(smem + 16 * i) = i32x4{0, 0, 0, 0};

  const float s_in = a.act_scale[a.in_scale];
  // staging: slice s -> registers -> LDS image
  i32x4 st[kStagePerThread];
  h8 pr[PRE ? 2 * kStagePerThread : 1];
  auto stage_load = [&](int s) {
#pragma unroll
    for (int k = 0; k < kStagePerThread; ++k) {
      int it = tid + kWgI8 * k;
      if (it >= kStageItems) it = kStageItems - 1;   // tail threads re-read a valid point (not stored)
      const int gc = it / kNLoc, p = it - gc * kNLoc, c16 = s * (kSliceCh / 16) + gc;
      if (PRE) {
        const _Float16* x = (const _Float16*)a.in + ((size_t)pos * (CIN / 8) + 2 * c16) * kNLoc * 8;
        pr[2 * k] = *(const h8*)(x + p * 8);
        pr[2 * k + 1] = *(const h8*)(x + kNLoc * 8 + p * 8);
      } else {
        st[k] = *(const i32x4*)((const int8_t*)a.in + (((size_t)pos * (CIN / 16) + c16) * kNLoc + p) * 16);
      }
    }
  };
  auto stage_store = [&](int s, char* img) {
#pragma unroll
    for (int k = 0; k < kStagePerThread; ++k) {
      const int it = tid + kWgI8 * k;
      if (it >= kStageItems) continue;
      const int gc = it / kNLoc, p = it - gc * kNLoc;
      i32x4 v;
      if (PRE) v = stage_pre(pr[2 * k], pr[2 * k + 1], a.scale_in, a.shift_in, (s * (kSliceCh / 16) + gc) * 16, s_in);
      else v = st[k];
      *(i32x4*)(img + (gc * kPadPts + pad_index(p)) * 16) = v;
    }
  };

  // this lane's board points: tile t = wid + 4 i, point 16 t + (lane & 15); points past the board read the image at
  // point 0's place (any in-range address) and are never stored
  int pidx[kTilesPerWave];
#pragma unroll
  for (int i = 0; i < kTilesPerWave; ++i) {
    const int loc = 16 * (wid + 4 * i) + (lane & 15);
    pidx[i] = (g * kPadPts + (loc < kNLoc ? pad_index(loc) : pad_index(0))) * 16;
  }
  const int ntile = wid + 4 * (kTilesPerWave - 1) < kTiles ? kTilesPerWave : kTilesPerWave - 1;   // wave-uniform

  i32x4 acc[kTilesPerWave][4];
#pragma unroll
  for (int i = 0; i < kTilesPerWave; ++i)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[i][ct] = i32x4{0, 0, 0, 0};

  __syncthreads();   // zeroed images before the first staged store
  stage_load(0);
  stage_store(0, smem);
  __syncthreads();
  const int8_t* wp = (const int8_t*)a.w + (size_t)cp * NS * KK * 4 * 1024 + lane * 16;
#pragma unroll 1
  for (int s = 0; s < NS; ++s) {
    if (s + 1 < NS) stage_load(s + 1);
    const char* img = smem + (s & 1) * kSliceBytes;
#pragma unroll 1
    for (int tap = 0; tap < KK; ++tap) {
      i32x4 A[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) A[ct] = *(const i32x4*)(wp + ((size_t)(s * KK + tap) * 4 + ct) * 1024);
      const int off = KW == 3 ? ((tap / 3 - 1) * kPad + (tap % 3 - 1)) * 16 : 0;
#pragma unroll
      for (int i = 0; i < kTilesPerWave; ++i) {
        if (i < ntile) {
          const i32x4 B = *(const i32x4*)(img + pidx[i] + off);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) acc[i][ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[ct], B, acc[i][ct], 0, 0, 0);
        }
      }
    }
    if (s + 1 < NS) stage_store(s + 1, smem + ((s + 1) & 1) * kSliceBytes);
    __syncthreads();
  }

  // epilogue: lane holds output channels c0 + r (r = 0..3) of board point loc, for every (tile, cout tile)
  const float s_out = (!OUT16 && (ACT || DUAL)) ? a.act_scale[a.out_scale] : 0.0f;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int c0 = cp * 64 + ct * 16 + 4 * g;
    const f32x4 sw = *(const f32x4*)(a.w_scale + c0);
    f32x4 mult, sc = {0, 0, 0, 0}, sh = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) mult[r] = s_in * sw[r];
    if (ACT || DUAL) {
      sc = *(const f32x4*)(a.scale_out + c0);
      sh = *(const f32x4*)(a.shift_out + c0);
    }
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
      const int loc = 16 * (wid + 4 * i) + (lane & 15);
      if (i >= ntile || loc >= kNLoc) continue;
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (float)acc[i][ct][r] * mult[r];
      const size_t o16 = (((size_t)pos * (COUT / 8) + (c0 >> 3)) * kNLoc + loc) * 8 + (c0 & 7);     // fp16 layout
      const size_t o8 = (((size_t)pos * (COUT / 16) + (c0 >> 4)) * kNLoc + loc) * 16 + (c0 & 15);   // int8 layout
      if (RES) {
        const h4 old = *(const h4*)((const _Float16*)a.out + o16);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)old[r];
      }
      if constexpr (OUT16 && (ACT || DUAL)) {
        h4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (_Float16)mish_f(v[r] * sc[r] + sh[r]);
        *(h4*)((_Float16*)(ACT ? a.out : (void*)a.out2) + o16) = o;
      } else if (ACT || DUAL) {
        unsigned u = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) u |= q8(mish_f(v[r] * sc[r] + sh[r]), s_out) << (8 * r);
        *(unsigned*)((int8_t*)(ACT ? a.out : a.out2) + o8) = u;
      }
      if (!ACT) *(h4*)((_Float16*)a.out + o16) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    }
  }
}

}  // namespace
}  // namespace p3
