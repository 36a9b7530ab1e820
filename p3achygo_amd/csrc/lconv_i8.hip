// lconv_i8.hip — the INT8 layer convs of the layer-wise trunks at their templated widths (P3HIP_FLAG_INT8) and the absmax
// reduction that calibrates the activation scales.  Numerics: DESIGN.md section 9.  The body, its operand layouts and
// its tiling: lconv_i8_core.h; the same body with the widths as launch arguments: lconv_i8_any.hip.
#include "lconv_i8_core.h"

namespace p3 {
namespace {

template <int KW, int CIN, int COUT, bool PRE, bool ACT, bool RES, bool DUAL>
__global__ void __launch_bounds__(kWgI8, 2) k_lconv_i8(LConvI8Args a) {
  lconv_i8_body<KW, FixedW<CIN>, FixedW<COUT>, PRE, ACT, RES, DUAL>(a, FixedW<CIN>{}, FixedW<COUT>{});
}

// Largest |v| of an fp16 tensor [npos][C / 8][361][8], v = the stored value or mish(bn(value)), folded into *amax as
// float bits by an integer atomicMax (all candidates are >= 0, so the result does not depend on the order)
__global__ void __launch_bounds__(kWgI8) k_absmax(AbsmaxArgs a) {
  const size_t n = (size_t)a.npos * (a.C / 8) * kNLoc;
  float m = 0.0f;
  for (size_t i = (size_t)blockIdx.x * kWgI8 + threadIdx.x; i < n; i += (size_t)gridDim.x * kWgI8) {
    const h8 v = *(const h8*)(a.in + i * 8);
    const int c0 = (int)((i / kNLoc) % (a.C / 8)) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = (float)v[j];
      if (a.scale) x = mish_f(x * a.scale[c0 + j] + a.shift[c0 + j]);
      m = fmaxf(m, fabsf(x));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  if ((threadIdx.x & 63) == 0) atomicMax(a.amax, __float_as_uint(m));
}

}  // namespace

template <int KW, int CIN, int COUT, bool PRE, bool ACT, bool RES, bool DUAL>
static hipError_t launch_t(const LConvI8Args& a, hipStream_t s) {
  constexpr size_t lds = 2 * kSliceBytes;
  static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
  hipLaunchKernelGGL((k_lconv_i8<KW, CIN, COUT, PRE, ACT, RES, DUAL>), dim3(a.npos * (COUT / 64)), dim3(kWgI8), lds, s, a);
  return hipGetLastError();
}

// the ten layer shapes and flag sets launch_lconv dispatches (kernels.hip)
hipError_t launch_lconv_i8(int kw, int cin, int cout, const LConvI8Args& a, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  const int f = (a.pre ? 8 : 0) | (a.act ? 4 : 0) | (a.res ? 2 : 0) | (a.dual ? 1 : 0);
#define P3_LCONV_I8(KW, CIN, COUT, PRE, ACT, RES, DUAL) \
  if (kw == KW && cin == CIN && cout == COUT && f == ((PRE ? 8 : 0) | (ACT ? 4 : 0) | (RES ? 2 : 0) | (DUAL ? 1 : 0))) \
    return launch_t<KW, CIN, COUT, PRE, ACT, RES, DUAL>(a, s);
  P3_LCONV_I8(1, 384, 192, true, true, false, false)     // btl reduce from the raw stream
  P3_LCONV_I8(1, 384, 192, false, true, false, false)    // btl reduce from the activated copy
  P3_LCONV_I8(1, 384, 192, true, false, false, true)     // nbt reduce (t raw + act1(t))
  P3_LCONV_I8(1, 384, 192, false, false, false, true)
  P3_LCONV_I8(3, 192, 192, false, true, false, false)    // inner conv, activated output
  P3_LCONV_I8(3, 192, 192, true, true, false, false)     // classic conv0 from the raw stream
  P3_LCONV_I8(3, 192, 192, false, false, true, false)    // classic conv1 (+x), last block
  P3_LCONV_I8(3, 192, 192, false, false, true, true)     // nbt conv2 / conv4, classic conv1 (+x, + next act)
  P3_LCONV_I8(1, 192, 384, false, false, true, false)    // expand + x
  P3_LCONV_I8(1, 192, 384, false, false, true, true)     // expand + x, + the next block's activated input
#undef P3_LCONV_I8
  return hipErrorInvalidValue;
}

// (a shape without a templated instantiation is a runtime launch, lconv_i8_any.hip)
const char* lconv_i8_kernel_name(int kw, int cin, int cout) {
  if (kw == 3 && cin == 192 && cout == 192) return "k_lconv_i8<3,192,192>";
  if (kw == 1 && cin == 384 && cout == 192) return "k_lconv_i8<1,384,192>";
  if (kw == 1 && cin == 192 && cout == 384) return "k_lconv_i8<1,192,384>";
  return lconv_i8_any_kernel_name(kw);
}

hipError_t launch_absmax(const AbsmaxArgs& a, int n_cu, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  const size_t n = (size_t)a.npos * (a.C / 8) * kNLoc;
  size_t grid = (n + kWgI8 - 1) / kWgI8;
  if (grid > (size_t)4 * n_cu) grid = (size_t)4 * n_cu;
  hipLaunchKernelGGL(k_absmax, dim3((unsigned)grid), dim3(kWgI8), 0, s, a);
  return hipGetLastError();
}

}  // namespace p3
