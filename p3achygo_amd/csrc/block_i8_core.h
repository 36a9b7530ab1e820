// block_i8_core.h — what the fused INT8 block kernels share (block_i8.hip at C = 256 / C_b = 128, block_i8_c128.hip at
// C = 128 / C_b = 64): the padded int8 image in LDS, the quantizer, the staging of 16 channels of x, and a wave's conv
// over 64 output channels and six 16-point tiles.  Numerics: DESIGN.md section 9 "Fused INT8 blocks"; the weight stream
// is pack_lconv_i8's (lconv_i8.h).
#pragma once
#include <stdint.h>

#include "conv_core.h"

namespace p3 {

typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace i8blk {

constexpr int kPad = 21;                        // padded board side
constexpr int kPadPts = kPad * kPad;            // 441
constexpr int kGroupBytes = kPadPts * 16;       // 16 channels of the padded board: 7,056
constexpr int kSliceBytes = 4 * kGroupBytes;    // a 64-channel K slice: 28,224
constexpr int kTiles = (kNLoc + 15) / 16;       // 23 point tiles
constexpr int kTilesPerWave = (kTiles + 3) / 4; // 6

__device__ __forceinline__ int pad_index(int loc) { return (loc / 19 + 1) * kPad + loc % 19 + 1; }

// q = clamp(rint(y / s), -127, 127); a zero scale (an all-zero tensor) quantizes everything to 0
__device__ __forceinline__ unsigned q8(float y, float s) {
  if (!(s > 0.0f)) return 0u;
  float q = __builtin_rintf(y / s);
  q = fminf(fmaxf(q, -127.0f), 127.0f);
  return (unsigned)((int)q) & 0xffu;
}

// 16 channels of one point from the raw fp16 stream, mish(bn0(.)) and quantized
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

// acc[i][ct] += W . a over NS 64-channel K slices of the image(s) at `img` and the KW x KW taps.  wp: this wave's
// output pass of the conv's weight stream plus lane * 16; the (slice, tap) steps lie 4 KB apart in it.
template <int KW, int NS>
__device__ __forceinline__ void conv_i8(i32x4 (&acc)[kTilesPerWave][4], const char* img, const int8_t* wp,
                                        const int (&pidx)[kTilesPerWave], int ntile) {
  constexpr int KK = KW * KW, NT = NS * KK;
  i32x4 A[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) A[ct] = *(const i32x4*)(wp + ct * 1024);
#pragma unroll 1
  for (int t = 0; t < NT; ++t) {
    const int tn = t + 1 < NT ? t + 1 : t;   // the last step re-reads its own fragments
    i32x4 An[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) An[ct] = *(const i32x4*)(wp + ((size_t)tn * 4 + ct) * 1024);
    const int s = t / KK, tap = t - s * KK;
    const int off = s * kSliceBytes + (KW == 3 ? ((tap / 3 - 1) * kPad + (tap % 3 - 1)) * 16 : 0);
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
      if (i < ntile) {
        const i32x4 B = *(const i32x4*)(img + pidx[i] + off);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[i][ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[ct], B, acc[i][ct], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) A[ct] = An[ct];
  }
}

}  // namespace i8blk
}  // namespace p3
