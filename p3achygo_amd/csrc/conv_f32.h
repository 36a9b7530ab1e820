// conv_f32.h — the fp32 plan of the conv trunks (include/p3hip.h P3HIP_FLAG_FP32): fp32 twins of the four kernels of
// conv_any.hip (stem, layer conv, per-position 1x1, broadcast dense).  Weights, activations, BN fold, mish and residual
// adds are fp32; every product runs on the f32-input MFMA v_mfma_f32_32x32x2_f32, which is bit-equal to an fmaf chain.
// Widths are launch arguments, multiples of 64 channels (engine.cpp WeightFile::pad_conv pads a file's C and C_b).
//
// Activation layout: that of the fp16 plans with 4-byte elements, [pos][C / 8][361][8] floats.  The head convs write
// hp as [pos][96 / 4][361][4], what k_heads reads.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace p3 {

constexpr int kF32MaxC = 512;

struct InitF32Args {
  const void* feats;    // npos x p3hip_features
  float* x;             // [npos][C / 8][361][8]
  int npos, C;
  const float* w;       // pack_conv_f32(init_conv.w, 25 taps, 15 -> 16 input planes, C)
  const float* game_w;  // [8][C]
  const float* game_b;  // [C]
};

// One conv of the layer-wise plan, and the per-position 1x1 convs as flag sets of it:
//   y = conv(in') [+ out], in' = mish(bn_in(in)) when pre
//   act 1: mish(bn_out(y)) stored instead of y; act 2: mish(y) (broadcast conv_first)
//   dual: y to `out` and mish(bn_out(y)) to `out2`
//   hp: the head convs, cout = 96 of a weight image padded to 128, y stored as [pos][96 / 4][361][4]
struct LConvF32Args {
  const float* in;
  float* out;
  float* out2;
  int npos, cin, cout;
  const float* w;       // pack_conv_f32
  int pre, act, res, dual, hp;
  const float *scale_in, *shift_in;
  const float *scale_out, *shift_out;
};

struct BDenseF32Args {
  const float* t;
  float* u;
  int npos, C;
  const float* w;       // pack_dense_f32
  const float* bias;    // [361]
  const float* scale;   // folded bn1 [C]
  const float* shift;
};

hipError_t launch_init_f32(const InitF32Args& a, int n_cu, hipStream_t s);
// kw 1 or 3; cin, cout multiples of 64 up to kF32MaxC (hp: cout = 128)
hipError_t launch_lconv_f32(int kw, const LConvF32Args& a, int n_cu, hipStream_t s);
const char* lconv_f32_kernel_name(int kw);
hipError_t launch_bdense_f32(const BDenseF32Args& a, int n_cu, hipStream_t s);

// Weight images.  The A operand of v_mfma_f32_32x32x2_f32 is one float per lane, A[row = lane & 31][k = lane >> 5]; a
// lane's four floats are the four k-steps of one group of 8 input channels, so that lane half h owns channels 4 h .. 4 h + 3
// of the group and k-step s multiplies channel 8 g + 4 h + s (the activations are read in the same order):
//   [cout / 64 passes][tap][cin / 8 groups g][2 cout tiles mt][64 lanes][4 steps s]
//       = W[tap][8 g + 4 (lane >> 5) + s][64 pass + 32 mt + (lane & 31)]
// W is HWIO flattened as [taps][cin][cout]; rows and columns beyond it are zero.
inline void pack_conv_f32(std::vector<float>& dst, const float* W, int taps, int cin, int cout, int cin_pad, int cout_pad) {
  for (int cp = 0; cp < cout_pad / 64; ++cp)
    for (int tap = 0; tap < taps; ++tap)
      for (int g = 0; g < cin_pad / 8; ++g)
        for (int mt = 0; mt < 2; ++mt)
          for (int lane = 0; lane < 64; ++lane)
            for (int s = 0; s < 4; ++s) {
              const int ci = 8 * g + 4 * (lane >> 5) + s, co = 64 * cp + 32 * mt + (lane & 31);
              dst.push_back(ci < cin && co < cout ? W[((size_t)tap * cin + ci) * cout + co] : 0.0f);
            }
}

// The broadcast dense W[361 i][361 j] as B operands, B[k = lane >> 5][col = lane & 31]:
//   [12 column tiles jt][46 groups g of 8 rows][64 lanes][4 steps s] = W[8 g + 4 (lane >> 5) + s][32 jt + (lane & 31)]
constexpr int kDenseF32Groups = 46, kDenseF32Tiles = 12;
inline void pack_dense_f32(std::vector<float>& dst, const float* W) {
  for (int jt = 0; jt < kDenseF32Tiles; ++jt)
    for (int g = 0; g < kDenseF32Groups; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int s = 0; s < 4; ++s) {
          const int i = 8 * g + 4 * (lane >> 5) + s, j = 32 * jt + (lane & 31);
          dst.push_back(i < 361 && j < 361 ? W[(size_t)i * 361 + j] : 0.0f);
        }
}

}  // namespace p3
