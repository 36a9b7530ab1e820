// block_i8.h — arguments and launcher of the fused INT8 block kernel (block_i8.hip, k_block_i8): C = 256 / C_b = 128 btl
// trunks (geometry <256,128>, P3HIP_FLAG_INT8_FUSED) and C = 128 / C_b = 64 btl trunks (geometry <128,64>,
// P3HIP_FLAG_INT8_C128).
// Numerics: DESIGN.md section 9 "Fused INT8 blocks".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p3 {

constexpr int kBlockI8MaxConvs = 5;   // reduce + up to three inner 3x3 + expand

// One btl block with `inner` 3x3 layers on the stored fp16 x [npos][C / 8][361][8], in place (C = 256, C_b = 128 or
// C = 128, C_b = 64):
//   a0 = q(mish(bn0(x)))                                  quantized with act_scale[q0]
//   conv j = 0 .. inner:  a_{j+1} = q(mish(bn_{j+1}(acc * (act_scale[q0 + j] * w_scale[j][c]))))   with act_scale[q0 + j + 1]
//   x <- fp16((float) x + acc * (act_scale[q0 + inner + 1] * w_scale[inner + 1][c]))
// w[j]: the conv's weights in pack_lconv_i8 order (lconv_i8.h); scale[0] / shift[0]: folded bn0 [C];
// scale[j] / shift[j], j >= 1: folded bn_j [C_b].
struct BlockI8Args {
  _Float16* x;
  int npos, inner;
  const int8_t* w[kBlockI8MaxConvs];
  const float* w_scale[kBlockI8MaxConvs];
  const float* scale[kBlockI8MaxConvs];
  const float* shift[kBlockI8MaxConvs];
  const float* act_scale;   // device array of activation scales (read at launch time: graph replays see new values)
  int q0;
};

// C = 256: 512-thread workgroups, one per CU; C = 128: 256-thread workgroups, two per CU; any other C is
// hipErrorInvalidValue (and has no name)
hipError_t launch_block_i8(int C, const BlockI8Args& a, int n_cu, hipStream_t s);
const char* block_i8_kernel_name(int C);   // "k_block_i8<256,128>", "k_block_i8<128,64>"

}  // namespace p3
