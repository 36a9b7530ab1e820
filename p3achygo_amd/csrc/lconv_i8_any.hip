// lconv_i8_any.hip — the INT8 layer conv with its widths as launch arguments (P3HIP_FLAG_INT8_ANY, DESIGN.md section 9
// "INT8 at any width"): k_lconv_i8_any<KW, PRE, ACT, RES, DUAL> runs the body of lconv_i8_core.h with cin and cout,
// multiples of 64, from the launch.  Same operand layouts, slice order, tap order and epilogue arithmetic as the
// templated k_lconv_i8, so on its ten shapes the results are equal bit for bit (P3HIP_CONV_ANY=1 compares).  Bounds: the
// grid is npos x cout / 64 workgroups and a workgroup of pass cp reads slices 0 .. cin / 64 - 1 of position pos:
// activations below (pos + 1) cin 361 bytes, weights below (cp + 1) (cin / 64) taps 4096 <= taps cin cout bytes, scales
// and BN below cout floats, outputs below (pos + 1) cout 361 elements.
#include "lconv_i8_core.h"

namespace p3 {
namespace {

// cin, cout: multiples of 64, with the launch
template <int KW, bool PRE, bool ACT, bool RES, bool DUAL>
__global__ void __launch_bounds__(kWgI8, 2) k_lconv_i8_any(LConvI8Args a, int cin, int cout) {
  lconv_i8_body<KW, RuntimeW, RuntimeW, PRE, ACT, RES, DUAL>(a, RuntimeW{cin}, RuntimeW{cout});
}

}  // namespace

template <int KW, bool PRE, bool ACT, bool RES, bool DUAL>
static hipError_t launch_any_t(int cin, int cout, const LConvI8Args& a, hipStream_t s) {
  hipLaunchKernelGGL((k_lconv_i8_any<KW, PRE, ACT, RES, DUAL>), dim3(a.npos * (cout / 64)), dim3(kWgI8), 2 * kSliceBytes, s, a,
                     cin, cout);
  return hipGetLastError();
}

// the same ten flag sets (what the btl, nbt and classic blocks produce) at any widths that are multiples of 64
hipError_t launch_lconv_i8_any(int kw, int cin, int cout, const LConvI8Args& a, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  if (cin < 64 || cout < 64 || cin % 64 != 0 || cout % 64 != 0) return hipErrorInvalidValue;
  const int f = (a.pre ? 8 : 0) | (a.act ? 4 : 0) | (a.res ? 2 : 0) | (a.dual ? 1 : 0);
#define P3_LCONV_I8_ANY(KW, PRE, ACT, RES, DUAL) \
  if (kw == KW && f == ((PRE ? 8 : 0) | (ACT ? 4 : 0) | (RES ? 2 : 0) | (DUAL ? 1 : 0))) \
    return launch_any_t<KW, PRE, ACT, RES, DUAL>(cin, cout, a, s);
  P3_LCONV_I8_ANY(1, true, true, false, false)     // btl reduce from the raw stream
  P3_LCONV_I8_ANY(1, false, true, false, false)    // btl reduce from the activated copy
  P3_LCONV_I8_ANY(1, true, false, false, true)     // nbt reduce (t raw + act1(t))
  P3_LCONV_I8_ANY(1, false, false, false, true)
  P3_LCONV_I8_ANY(3, false, true, false, false)    // inner conv, activated output
  P3_LCONV_I8_ANY(3, true, true, false, false)     // classic conv0 from the raw stream
  P3_LCONV_I8_ANY(3, false, false, true, false)    // classic conv1 (+x), last block
  P3_LCONV_I8_ANY(3, false, false, true, true)     // nbt conv2 / conv4, classic conv1 (+x, + next act)
  P3_LCONV_I8_ANY(1, false, false, true, false)    // expand + x
  P3_LCONV_I8_ANY(1, false, false, true, true)     // expand + x, + the next block's activated input
#undef P3_LCONV_I8_ANY
  return hipErrorInvalidValue;
}

const char* lconv_i8_any_kernel_name(int kw) { return kw == 3 ? "k_lconv_i8_any<3>" : "k_lconv_i8_any<1>"; }

}  // namespace p3
