// transformer_core.h — what the fp16 transformer kernels for gfx950 (v_mfma_f32_16x16x32_f16) are made of, written once
// for the 64-token launches (transformer.hip) and the split ones (transformer_split.hip): the device helpers and the
// launchers' host helpers here, and the three kernel bodies in transformer_{qkv,attn,ffn}_body.inc, which both units
// include as text inside their kernels (why text and not functions: the note at the end of this comment).
//
// NT is the number of 16-token tiles of a qkv / ffn workgroup: 4 in transformer.hip, 1 and 2 in transformer_split.hip.
// Per token and per query the bodies do the same loads, the same MFMA chain in the same K order, the same RMSNorm
// partial sums over the same C / 4 channels and the same two __shfl_xor, the same fp32 expressions and the same
// roundings whatever NT and whatever part of the query tiles a workgroup takes: that is what lets the low-latency plan
// return the default plan's bits (tests/test_low_latency_tfm_gpu.py).
//
// The residual stream keeps the conv trunk's layout, [pos][Cs / 8][361][8] fp16 (kernels.h), Cs = tfm_stream_width(C):
// the model's C channels are channels 0..C-1, channels C..Cs-1 are the zero padding the stem leaves and no kernel here
// writes.  Tokens are s = 19 row + col.  qkv and ffn see the batch as one [npos * 361][C] matrix: a token tile may span
// two positions.  Accumulation, RMSNorm, RoPE, softmax and SiLU are fp32; what goes between kernels, and every MFMA
// operand, is fp16.  Every element offset into q, k, v, o and x is computed in 64 bits.
//
// Text, not functions: a body called from a thin __global__ wrapper, force-inlined, is optimised once on its own and
// once more inside the kernel, and that changed the instruction text of all 88 code objects (k_tfm_ffn<384> to 512
// VGPRs and scratch).  Included as text a body is compiled exactly as when each file held its own copy: every code
// object keeps its instructions and registers (tools/kernel_text_diff.py compares two builds).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "transformer.h"

namespace p3 {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

static __device__ inline f32x4 mfma(const h8& a, const h8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// address of channel c of token g (= pos * 361 + s) in the residual stream of width Cs
template <int Cs>
static __device__ inline size_t x_index(int g, int c) {
  const int p = g / kTfmL, s = g - p * kTfmL;
  return (((size_t)p * (Cs / 8) + (c >> 3)) * kTfmL + s) * 8 + (c & 7);
}

// D^T tile = W^T . T^T for output-channel tile ct and the NT 16-token tiles of the workgroup:
// acc[tt][i] = sum_k W[k][16 ct + 4 g + i] * T[16 tt + (lane & 15)][k], g = lane >> 4, every tile's chain in the K order
// st = 0 .. NST - 1.  W is packed as MFMA A fragments [ct][k32 step][64 lanes][8] (engine.cpp pack_afrag); T is an LDS
// tile with rows of `ld` halves.
template <int NST, int NT>
static __device__ inline void gemm_tile(const h8* __restrict__ wpack, int ct, const _Float16* t, int ld, f32x4 acc[NT]) {
  const int lane = threadIdx.x & 63;
  for (int tt = 0; tt < NT; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < NST; ++st) {
    const h8 a = wpack[((size_t)ct * NST + st) * 64 + lane];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
      const h8 b = *reinterpret_cast<const h8*>(t + (16 * tt + (lane & 15)) * ld + 32 * st + 8 * (lane >> 4));
      acc[tt] = mfma(a, b, acc[tt]);
    }
  }
}

// RMSNorm of the 16 NT x C fp32 rows `src(r, c)` into the fp16 LDS tile dst of rows C + 8, for the threads
// 0 .. 64 NT - 1 (whole waves: 4 threads per token, C / 4 channels each).  eps = 1e-6: the keras.layers.RMSNormalization
// default, which the reference does not override (not verified against Keras itself; at these magnitudes its effect is
// far below the engine's tolerance).
template <int C, class Src>
static __device__ inline void rms_rows(Src src, const float* __restrict__ scale, _Float16* dst) {
  constexpr int P = C / 4;
  const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
  float v[P];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    v[j] = src(r, P * q + j);
    ss += v[j] * v[j];
  }
  ss += __shfl_xor(ss, 1);
  ss += __shfl_xor(ss, 2);
  const float inv = rsqrtf(ss * (1.0f / C) + 1e-6f);
#pragma unroll
  for (int j = 0; j < P; ++j) dst[r * (C + 8) + P * q + j] = (_Float16)(v[j] * inv * scale[P * q + j]);
}

// RoPE.call on the lane's two pairs, x'[2j] = x[2j] cos + x[2j+1] sin, x'[2j+1] = x[2j] sin - x[2j+1] cos (a reflection),
// with the contraction written out and the compiler's own switched off: both products of x'[0] rounded and added, the
// second product of x'[1], x'[2] and x'[3] rounded and the first fused.  Who uses it and why: transformer_qkv_body.inc.
static __device__ inline f32x4 rope4(const f32x4& y, const float* cs, const float* sn) {
#pragma clang fp contract(off)
  const float p0 = y[0] * cs[0], p1 = y[1] * sn[0];
  f32x4 z;
  z[0] = p0 + p1;
  z[1] = __builtin_fmaf(y[0], sn[1], -(y[1] * cs[1]));
  z[2] = __builtin_fmaf(y[2], cs[2], y[3] * sn[2]);
  z[3] = __builtin_fmaf(y[2], sn[3], -(y[3] * cs[3]));
  return z;
}

// ---- host side of the launchers -----------------------------------------------------------------------
// workgroups of a qkv / ffn launch of `tokens` tokens each
static inline int token_tiles(int npos, int tokens) { return (int)(((long)npos * kTfmL + tokens - 1) / tokens); }

// every supported model width C (multiples of 32, 64..384) as a compile-time constant
template <class F>
static hipError_t dispatch_c(int C, F&& f) {
  switch (C) {
#define P3_TFM_C(c) case c: return f(std::integral_constant<int, c>{});
    P3_TFM_C(64) P3_TFM_C(96) P3_TFM_C(128) P3_TFM_C(160) P3_TFM_C(192) P3_TFM_C(224)
    P3_TFM_C(256) P3_TFM_C(288) P3_TFM_C(320) P3_TFM_C(352) P3_TFM_C(384)
#undef P3_TFM_C
    default: return hipErrorInvalidValue;
  }
}

}  // namespace p3
