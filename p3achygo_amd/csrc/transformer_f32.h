// transformer_f32.h — the fp32 plan of the transformer trunks (include/p3hip.h P3HIP_FLAG_FP32_TFM): fp32 twins of the
// three kernels of transformer.hip.  Weights, the residual stream, q / k / v / o, the softmax numerators and
// silu(gate) * up are fp32; every product runs on the f32-input MFMA v_mfma_f32_16x16x4_f32.  No fp16 value exists in
// the pass.  The model width C and the head width D are launch arguments (transformer.h tfm_supported).
//
// Layouts: those of transformer.h with 4-byte elements.  x is [pos][Cs / 8][361][8] floats, Cs = tfm_stream_width(C)
// (what k_init_f32 writes and the fp32 head convs read); q, k, v are [pos][head][384][D] floats with rows 361..383 zero;
// o is [pos][361][C] floats.  Every element offset into them is formed in size_t.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "transformer.h"

namespace p3 {

struct TfmQkvF32Args {
  const float* x;
  float *q, *k, *v;
  int npos, C, D;
  const float* rms_scale;     // rms_in [C]
  const float* wqkv;          // pack_tfm_f32 of [Wq | Wk | Wv]: N = 3 C, K = C
  const float *rope_cos, *rope_sin;   // [361][D]
};
struct TfmAttnF32Args {
  const float *q, *k, *v;
  float* o;
  int npos, heads;
};
struct TfmFfnF32Args {
  const float* o;
  float* x;                   // read as the residual, channels 0..C-1 written
  int npos, C;
  const float* wo;            // N = C, K = C
  const float* rms_scale;     // rms_out [C]
  const float* wgu;           // [Wgate | Wup]: N = 4 C, K = C
  const float* wdown;         // N = C, K = 2 C
};

// anything outside tfm_supported(C, C / D) returns hipErrorInvalidValue
hipError_t launch_tfm_qkv_f32(const TfmQkvF32Args& a, hipStream_t s);
hipError_t launch_tfm_attn_f32(int D, const TfmAttnF32Args& a, hipStream_t s);
hipError_t launch_tfm_ffn_f32(const TfmFfnF32Args& a, hipStream_t s);
const char* tfm_attn_f32_kernel_name();

// Weight image of a GEMM with the Keras (in, out) matrix W[K][ld], columns col0 .. col0 + N - 1.  The A operand of
// v_mfma_f32_16x16x4_f32 is one float per lane, A[row = lane & 15][k = lane >> 4].  A lane's eight floats are the eight
// MFMAs of one step of 32 input channels: MFMA e of step st multiplies channel 32 st + 8 (lane >> 4) + e (the
// activations are read from LDS in the same order, two 16-byte reads per step), so the image is
//   [N / 16 cout tiles ct][K / 32 steps st][64 lanes][8 e] = W[32 st + 8 (lane >> 4) + e][col0 + 16 ct + (lane & 15)]
// the fp16 plan's fragment order (engine.cpp pack_afrag) with 4-byte elements.
inline void pack_tfm_f32(std::vector<float>& dst, const float* W, int K, int N, int ld, int col0) {
  for (int ct = 0; ct < N / 16; ++ct)
    for (int st = 0; st < K / 32; ++st)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e)
          dst.push_back(W[(size_t)(32 * st + 8 * (lane >> 4) + e) * ld + col0 + 16 * ct + (lane & 15)]);
}

}  // namespace p3
