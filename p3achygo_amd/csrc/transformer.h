// transformer.h — argument structs and launchers of the transformer trunk (transformer.hip), shared with engine.cpp.
#pragma once
#include <hip/hip_runtime.h>

namespace p3 {

constexpr int kTfmL = 361;       // tokens
constexpr int kTfmLPad = 384;    // rows of a head's q / k / v (rows 361.. stay zero)

// The supported set (include/p3hip.h): model width C a multiple of 32 with 64 <= C <= 384, head width C / heads 32 or
// 64, every block alike.  The SwiGLU width is 2 C.  The residual stream is the smallest of 128, 256, 384 that holds C.
constexpr int kTfmMinC = 64, kTfmMaxC = 384;
inline bool tfm_supported(int C, int heads) {
  if (C < kTfmMinC || C > kTfmMaxC || C % 32 != 0 || heads < 1 || C % heads != 0) return false;
  const int D = C / heads;
  return D == 32 || D == 64;
}
constexpr int tfm_stream_width(int C) { return C <= 128 ? 128 : (C <= 256 ? 256 : 384); }

// Weight layout of every GEMM: MFMA 16x16x32 A fragments [N / 16 cout tiles][K / 32 steps][64 lanes][8] fp16 with
// element e of lane l = W[32 step + 8 (l >> 4) + e][16 tile + (l & 15)], W the Keras (in, out) matrix (engine.cpp).
struct TfmQkvArgs {
  const _Float16* x;          // residual stream [pos][Cs / 8][361][8]
  _Float16 *q, *k, *v;        // [pos][head][384][D]
  int npos;
  const float* rms_scale;     // rms_in [C]
  const void* wqkv;           // [Wq | Wk | Wv]: N = 3 C, K = C
  const float *rope_cos, *rope_sin;   // [361][D]
};
struct TfmAttnArgs {
  const _Float16 *q, *k, *v;
  _Float16* o;                // [pos][361][C], head h in channels D h ..
  int npos;
  int heads;
};
struct TfmFfnArgs {
  const _Float16* o;
  _Float16* x;                // read as the residual, channels 0..C-1 written
  int npos;
  const void* wo;             // N = C, K = C
  const float* rms_scale;     // rms_out [C]
  const void* wgu;            // [Wgate | Wup]: N = 4 C, K = C
  const void* wdown;          // N = C, K = 2 C
};

// C: model width, D: head width (tfm_supported(C, C / D)); anything else returns hipErrorInvalidValue
hipError_t launch_tfm_qkv(int C, int D, const TfmQkvArgs& a, hipStream_t s);
hipError_t launch_tfm_attn(int D, const TfmAttnArgs& a, hipStream_t s);
hipError_t launch_tfm_ffn(int C, const TfmFfnArgs& a, hipStream_t s);

}  // namespace p3
