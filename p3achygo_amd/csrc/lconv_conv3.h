// lconv_conv3.h — launchers of the two boundary convs of P3HIP_FLAG_INT8_CONV3 (lconv_conv3.hip, DESIGN.md section 9
// "INT8 for the 3x3 convs only"): a btl / nbt block's 3x3 convs run on int8, its 1x1 convs in fp16, and the conv on
// either side of that boundary stores its activated output in the other side's format.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lconv_i8.h"

namespace p3 {

// The fp16 1x1 reduce in front of the first 3x3 (k_lconv's body): `act`, or the second output of `dual`, is stored as
// q8(mish(bn_out(y)), act_scale[out_scale]) in the int8 layout [npos][cout / 16][361][16], quantized from the fp32
// value.  dual's raw output stays fp16.  Flag sets: (pre or not) x (act | dual), kw = 1.  any: widths as launch arguments
// (k_lconv_q8_any), else the templated 384 -> 192 (k_lconv_q8); anything else: hipErrorInvalidValue
hipError_t launch_lconv_q8(bool any, int kw, int cin, int cout, const LConvArgs& a, const float* act_scale, int out_scale,
                           int n_cu, hipStream_t s);
// The int8 3x3 in front of the fp16 1x1 expand (k_lconv_i8's body): `act` stores (_Float16) mish(bn_out(y)) in the fp16
// layout to `out`; res + dual store the raw fp16 sum to `out` and that fp16 activated tensor to `out2`.  kw = 3, input
// int8 (no pre).  any: k_lconv_i8_f16_any, else the templated 192 -> 192 (k_lconv_i8_f16)
hipError_t launch_lconv_i8_f16(bool any, int kw, int cin, int cout, const LConvI8Args& a, hipStream_t s);

}  // namespace p3
