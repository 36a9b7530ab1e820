// conv_any.hip — gfx950 kernels of the layer-wise conv trunk at any width from 64 to 512 channels (conv_any.h).
//
// They are the kernels of kernels.hip with the channel counts turned from template arguments into launch arguments:
// entry points over the same bodies (layer_kernels.h), so the K-slice loop count, the output pass count and the layout
// strides are runtime values, in units of 64 channels.  What stays a template argument is what changes the
// instruction stream (kernel size, prologue / epilogue flags, slice and pass width).  One kernel per flag set serves
// every width; the results are bit for bit those of the templated kernels (P3HIP_CONV_ANY=1 runs the C = 384 and
// classic C = 192 trunks through these; tests/test_conv_widths_gpu.py compares).
#include "conv_any.h"

#include <hip/hip_runtime.h>

#include <cstdlib>

#include "launch_util.h"
#include "layer_kernels.h"

namespace p3 {

namespace {

struct InitAnyArgs { InitArgs a; int C; };
struct Conv1x1AnyArgs { Conv1x1Args a; int cin, cout; };
struct LConvAnyArgs { LConvArgs a; int nip, ncp; };   // input slices / output passes of 64 channels
struct BDenseAnyArgs { BDenseArgs a; int C; };

// LDS of k_bdense_any: Tt, the ring, the dense bias [384] and the folded bn1 [2][kConvAnyMaxC]; one workgroup per CU
constexpr size_t kBDenseAnyLds = kTtBytes + ring_bytes(128) + (384 + 2 * kConvAnyMaxC) * 4;
static_assert(kBDenseAnyLds <= 160 * 1024, "k_bdense_any: LDS of one CU");

}  // namespace

template <int CP>
__global__ void __launch_bounds__(kWG, 2) k_init_any(InitAnyArgs aa) {
  static_assert(kConvAnyMaxC <= kWG, "the game-state dense: one thread per channel");
  init_body<CP>(aa.a, RuntimeW{aa.C});
}

template <int CB, int CP, bool PRE, int EPI>
__global__ void __launch_bounds__(kWG, 2) k_conv1x1_any(Conv1x1AnyArgs aa) {
  conv1x1_body<CB, CP, PRE, EPI>(aa.a, RuntimeW{aa.cin}, RuntimeW{aa.cout});
}

// the layer conv exists in its shipped 4-wave form only (two 256-thread workgroups per CU)
template <int KW, bool PRE, bool ACT, bool RES, bool DUAL>
__global__ void __launch_bounds__(256, 2) k_lconv_any(LConvAnyArgs aa) {
  lconv_body<KW, PRE, ACT, RES, DUAL, 4>(aa.a, RuntimeW{aa.nip}, RuntimeW{aa.ncp});
}

__global__ void __launch_bounds__(kWG, 2) k_bdense_any(BDenseAnyArgs aa) {
  bdense_body(aa.a, RuntimeW{aa.C});
}

// =======================================================================================
// Host-side launchers
// =======================================================================================
namespace {

bool width_ok(int c) { return c >= 64 && c <= kConvAnyMaxC && c % 64 == 0; }

template <int CP>
hipError_t launch_init_cp(const InitAnyArgs& a, int grid, hipStream_t s) {
  using G = Geo<1, 16, 5>;
  constexpr size_t lds = G::ACT_BYTES + ring_bytes(CP) + kConvAnyMaxC * 4;   // + the game-state bias vector
  static_assert(2 * lds <= 160 * 1024, "k_init_any: two workgroups per CU");
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_init_any<CP>, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((k_init_any<CP>), dim3(grid), dim3(kWG), lds, s, a);
  return hipGetLastError();
}

template <int CB, int CP, bool PRE, int EPI>
hipError_t launch_conv1x1_t(const Conv1x1AnyArgs& a, int n_cu, hipStream_t s) {
  using G = Geo<128 / CB, CB, 1>;
  const int grid = conv_split_grid(a.a.npos, 128 / CB, (a.cout + CP - 1) / CP, n_cu);
  constexpr size_t lds = G::ACT_BYTES + ring_bytes(CP);
  static_assert(lds <= 160 * 1024, "k_conv1x1_any: LDS of one CU");
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_conv1x1_any<CB, CP, PRE, EPI>, lds); e != hipSuccess) return e;
  hipLaunchKernelGGL((k_conv1x1_any<CB, CP, PRE, EPI>), dim3(grid), dim3(kWG), lds, s, a);
  return hipGetLastError();
}

template <int KW, bool PRE, bool ACT, bool RES, bool DUAL>
hipError_t launch_lconv_t(const LConvArgs& a, int cin, int cout, int n_cu, hipStream_t s) {
  using G = Geo<1, 64, KW, 4, KW == 3 ? 2 : kKMS>;
  const int grid = conv_split_grid(a.npos, 1, cout / 64, 2 * n_cu);   // two workgroups per CU
  constexpr size_t lds = G::ACT_BYTES + ring_bytes(64, G::KMS);
  static_assert(2 * lds <= 160 * 1024, "k_lconv_any: two workgroups per CU");
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_lconv_any<KW, PRE, ACT, RES, DUAL>, lds); e != hipSuccess) return e;
  LConvAnyArgs b{a, cin / 64, cout / 64};
  b.a.nms_total = a.nms_total * (kKMS / G::KMS);   // the host counts macro-steps of kKMS k16-steps
  static const bool turns = getenv("P3HIP_NO_PAIR_TURNS") == nullptr;
  b.a.pair_split = (turns && grid > n_cu) ? n_cu : 0;
  hipLaunchKernelGGL((k_lconv_any<KW, PRE, ACT, RES, DUAL>), dim3(grid), dim3(256), lds, s, b);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_init_any(int C, const InitArgs& a, int grid, hipStream_t s) {
  if (!width_ok(C)) return hipErrorInvalidValue;
  const InitAnyArgs b{a, C};
  return conv_any_init_pass(C) == 128 ? launch_init_cp<128>(b, grid, s) : launch_init_cp<64>(b, grid, s);
}

hipError_t launch_conv1x1_any(int C, int which, const Conv1x1Args& a, int n_cu, hipStream_t s) {
  if (!width_ok(C) || which < 0 || which > 2) return hipErrorInvalidValue;
  const Conv1x1AnyArgs b{a, C, which == 2 ? 96 : C};
  if (conv_any_slice(C) == 128) {
    if (which == 0) return launch_conv1x1_t<128, 128, true, 0>(b, n_cu, s);
    if (which == 1) return launch_conv1x1_t<128, 128, false, 1>(b, n_cu, s);
    return launch_conv1x1_t<128, 64, false, 2>(b, n_cu, s);
  }
  if (which == 0) return launch_conv1x1_t<64, 64, true, 0>(b, n_cu, s);
  if (which == 1) return launch_conv1x1_t<64, 64, false, 1>(b, n_cu, s);
  return launch_conv1x1_t<64, 64, false, 2>(b, n_cu, s);
}

// the flag sets of the layer-wise plan (engine.cpp build_plan); f = pre, act, res, dual
hipError_t launch_lconv_any(int kw, int cin, int cout, const LConvArgs& a, int n_cu, hipStream_t s) {
  if (!width_ok(cin) || !width_ok(cout)) return hipErrorInvalidValue;
  const int f = (a.pre ? 8 : 0) | (a.act ? 4 : 0) | (a.res ? 2 : 0) | (a.dual ? 1 : 0);
#define P3_LCONV_ANY(KW, PRE, ACT, RES, DUAL) \
  if (kw == KW && f == ((PRE ? 8 : 0) | (ACT ? 4 : 0) | (RES ? 2 : 0) | (DUAL ? 1 : 0))) \
    return launch_lconv_t<KW, PRE, ACT, RES, DUAL>(a, cin, cout, n_cu, s);
  P3_LCONV_ANY(1, true, true, false, false)     // btl reduce from the raw stream
  P3_LCONV_ANY(1, false, true, false, false)    // btl reduce from the activated copy
  P3_LCONV_ANY(1, true, false, false, true)     // nbt reduce (t raw + act1(t))
  P3_LCONV_ANY(1, false, false, false, true)
  P3_LCONV_ANY(3, false, true, false, false)    // inner conv, activated output
  P3_LCONV_ANY(3, true, true, false, false)     // classic conv0 from the raw stream
  P3_LCONV_ANY(3, false, false, true, false)    // classic conv1 (+x), last block
  P3_LCONV_ANY(3, false, false, true, true)     // nbt conv2 / conv4, classic conv1 (+x, + next act)
  P3_LCONV_ANY(1, false, false, true, false)    // expand + x
  P3_LCONV_ANY(1, false, false, true, true)     // expand + x, + the next block's activated input
#undef P3_LCONV_ANY
  return hipErrorInvalidValue;
}

const char* lconv_any_kernel_name(int kw) { return kw == 3 ? "k_lconv_any<3>" : "k_lconv_any<1>"; }

hipError_t launch_bdense_any(int C, const BDenseArgs& a, int grid, hipStream_t s) {
  if (!width_ok(C)) return hipErrorInvalidValue;
  static AttrOnce once;
  if (hipError_t e = ensure_lds(once, k_bdense_any, kBDenseAnyLds); e != hipSuccess) return e;
  const BDenseAnyArgs b{a, C};
  hipLaunchKernelGGL(k_bdense_any, dim3(grid), dim3(kWG), kBDenseAnyLds, s, b);
  return hipGetLastError();
}

}  // namespace p3
