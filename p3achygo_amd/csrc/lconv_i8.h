// lconv_i8.h — argument structs, launchers and the host-side weight quantizer of the INT8 layer convs (lconv_i8.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <vector>

namespace p3 {

// One INT8 conv layer of the layer-wise path.  The input is the activated tensor as int8 [npos][CIN/16][361][16]
// quantized with act_scale[in_scale], or (pre) the raw fp16 stream [npos][CIN/8][361][8], activated and quantized while
// staging.  y = acc * (act_scale[in_scale] * w_scale[c]) in fp32, then as LConvArgs: act stores
// q(mish(bn_out(y))) as int8 to `out`; res adds the fp16 `out` in place; dual stores the raw y as fp16 to `out` and
// q(mish(bn_out(y))) as int8 to `out2`.  Outputs are quantized with act_scale[out_scale] (the consumer's scale).
struct LConvI8Args {
  const void* in;
  void* out;
  int8_t* out2;
  int npos;
  const int8_t* w;          // quantized weights, pack_lconv_i8 order
  const float* w_scale;     // [COUT] per output channel
  const float* act_scale;   // device array of activation scales (read at launch time: graph replays see new values)
  int in_scale, out_scale;
  int pre, act, res, dual;
  const float *scale_in, *shift_in;    // folded BN of the prologue   [CIN]
  const float *scale_out, *shift_out;  // folded BN of the epilogue   [COUT]
};

// max |v| over an fp16 tensor [npos][C/8][361][8]; v = mish(scale * x + shift) per channel when scale != null.
// Folded into *amax (float bits, atomicMax).
struct AbsmaxArgs {
  const _Float16* in;
  int npos, C;
  const float *scale, *shift;
  unsigned* amax;
};

// k_lconv_i8<KW, CIN, COUT, ..>: the ten templated shapes of C = 384 / C_b = 192 and classic C = 192
hipError_t launch_lconv_i8(int kw, int cin, int cout, const LConvI8Args& a, hipStream_t s);
// k_lconv_i8_any<KW, ..>: the same body with cin and cout (multiples of 64) as launch arguments, kw 1 or 3 and the flag
// sets the three block kinds produce; anything else: hipErrorInvalidValue.  Bit for bit the templated kernels' results
// on their shapes (P3HIP_FLAG_INT8_ANY, DESIGN.md section 9 "INT8 at any width")
hipError_t launch_lconv_i8_any(int kw, int cin, int cout, const LConvI8Args& a, hipStream_t s);
hipError_t launch_absmax(const AbsmaxArgs& a, int n_cu, hipStream_t s);
const char* lconv_i8_kernel_name(int kw, int cin, int cout);   // a shape without an instantiation: the runtime kernel's
const char* lconv_i8_any_kernel_name(int kw);                  // "k_lconv_i8_any<3>" / "k_lconv_i8_any<1>"

// Symmetric per-output-channel quantization of a conv's weights W (HWIO flattened [taps][cin][cout]):
//   s_w[c] = max_k |W[k][c]| / 127,  q = clamp(rint(W / s_w[c]), -127, 127)   (s_w = 0: q = 0)
// and the stream k_lconv_i8 reads: [cout pass of 64][K slice of 64][tap][cout tile of 16][64 lanes][16 bytes], lane l
// of a fragment holding q[tap][16 * (l >> 4) + j of the slice][cout 16 tile + (l & 15)], j = 0..15.
inline void pack_lconv_i8(std::vector<int8_t>& q, std::vector<float>& s_w, const float* W, int taps, int cin, int cout) {
  s_w.assign(cout, 0.0f);
  for (int c = 0; c < cout; ++c) {
    float m = 0.0f;
    for (int k = 0; k < taps * cin; ++k) m = std::fmax(m, std::fabs(W[(size_t)k * cout + c]));
    s_w[c] = m / 127.0f;
  }
  q.clear();
  q.reserve((size_t)taps * cin * cout);
  for (int cp = 0; cp < cout / 64; ++cp)
    for (int s = 0; s < cin / 64; ++s)
      for (int tap = 0; tap < taps; ++tap)
        for (int ct = 0; ct < 4; ++ct)
          for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 16; ++j) {
              const int co = cp * 64 + ct * 16 + (l & 15), ci = s * 64 + 16 * (l >> 4) + j;
              const float sw = s_w[co];
              float v = 0.0f;
              if (sw > 0.0f) {
                v = std::rint(W[((size_t)tap * cin + ci) * cout + co] / sw);
                v = std::fmin(std::fmax(v, -127.0f), 127.0f);
              }
              q.push_back((int8_t)v);
            }
}

}  // namespace p3
