// transformer.h — argument structs and launchers of the transformer trunk (transformer.hip), shared with engine.cpp.
#pragma once
#include <hip/hip_runtime.h>

namespace p3 {

constexpr int kTfmC = 96;        // model width (b14d96h3_transformer)
constexpr int kTfmHeads = 3;
constexpr int kTfmD = 32;        // head width
constexpr int kTfmF = 2 * kTfmC; // SwiGLU width
constexpr int kTfmL = 361;       // tokens
constexpr int kTfmLPad = 384;    // rows of a head's q / k / v (rows 361.. stay zero)

// Weight layout of every GEMM: MFMA 16x16x32 A fragments [N / 16 cout tiles][K / 32 steps][64 lanes][8] fp16 with
// element e of lane l = W[32 step + 8 (l >> 4) + e][16 tile + (l & 15)], W the Keras (in, out) matrix (engine.cpp).
struct TfmQkvArgs {
  const _Float16* x;          // residual stream [pos][128 / 8][361][8]
  _Float16 *q, *k, *v;        // [pos][head][384][32]
  int npos;
  const float* rms_scale;     // rms_in [96]
  const void* wqkv;           // [Wq | Wk | Wv]: N = 288, K = 96
  const float *rope_cos, *rope_sin;   // [361][32]
};
struct TfmAttnArgs {
  const _Float16 *q, *k, *v;
  _Float16* o;                // [pos][361][96], head h in channels 32 h ..
  int npos;
};
struct TfmFfnArgs {
  const _Float16* o;
  _Float16* x;                // read as the residual, channels 0..95 written
  int npos;
  const void* wo;             // N = 96, K = 96
  const float* rms_scale;     // rms_out [96]
  const void* wgu;            // [Wgate | Wup]: N = 384, K = 96
  const void* wdown;          // N = 96, K = 192
};

hipError_t launch_tfm_qkv(const TfmQkvArgs& a, hipStream_t s);
hipError_t launch_tfm_attn(const TfmAttnArgs& a, hipStream_t s);
hipError_t launch_tfm_ffn(const TfmFfnArgs& a, hipStream_t s);

}  // namespace p3
