// lconv_conv3.hip — the boundary convs of P3HIP_FLAG_INT8_CONV3 (lconv_conv3.h): entry points over the bodies of
// layer_kernels.h (lconv_body with the quantizing output policy below) and lconv_i8_core.h (lconv_i8_body with OUT16), at
// the templated C = 384 / C_b = 192 widths and with the widths as launch arguments.  Both forms run the same slices in the
// same order with the same epilogue arithmetic: equal bit for bit (P3HIP_CONV_ANY=1 compares).
#include "lconv_conv3.h"

#include <cstdlib>

#include "launch_util.h"
#include "lconv_i8_core.h"

namespace p3 {
namespace {

// lconv_body's Q: the activated accumulators (fp32, after activate()) quantized with act_scale[out_scale], the consumer's
// scale, and stored in the int8 layout [pos][COUT / 16][361][16].  A lane holds, per location tile j and register quad k,
// channels c0 + 8 k .. + 3 of one board point (conv_core.h acc_chan): one 4-byte store each, lconv_i8_core.h's o8
// addressing.  One position per workgroup (NW = 4).  Bounds: c < COUT and loc < 361, so a store ends below
// (pos0 + 1) COUT 361 bytes.  Every tile of a 4-wave workgroup has valid rows, so each wave issues all 8 NTn stores
// (the ring's vmcnt bookkeeping in lconv_body counts them).
struct Q8Out {
  static constexpr bool on = true;
  const float* act_scale;
  int out_scale;
  template <class G, int CP, int NTn>
  __device__ __forceinline__ void store(f32x16 (&acc)[2][NTn], void* out, int COUT, int pos0, int cofs) const {
    using T = Tiling<G, CP>;
    static_assert(G::NPOS == 1 && T::LG * NTn == G::NT_TOTAL, "one position, no padded tile");
    const float s = act_scale[out_scale];
    const int lane = launder(threadIdx.x & 63);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lg = wid / T::CG;
    const int lr = lane & 31, h = lane >> 5;
    const int c0 = cofs + cg_of<G, CP>() * 64 + h * 4;
    int8_t* base = (int8_t*)out + (size_t)pos0 * COUT * kNLoc;   // 64-bit per position, 32-bit inside it
#pragma unroll
    for (int j = 0; j < NTn; ++j) {
      const int t = lg + j * T::LG;
      int loc;
      const bool ok = row_valid<G::S>(t * 32 + lr, loc);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = c0 + 8 * k;
        unsigned u = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) u |= q8(acc[k >> 2][j][(k & 3) * 4 + i], s) << (8 * i);
        if (ok) *(unsigned*)(base + (uint32_t)(((c >> 4) * kNLoc + loc) * 16 + (c & 15))) = u;
      }
    }
  }
};

struct LConvQArgs { LConvArgs a; Q8Out q; };
struct LConvQAnyArgs { LConvArgs a; Q8Out q; int nip, ncp; };   // input slices / output passes of 64 channels

template <int KW, int CIN, int COUT, bool PRE, bool ACT, bool DUAL>
__global__ void __launch_bounds__(256, 2) k_lconv_q8(LConvQArgs aa) {
  lconv_body<KW, PRE, ACT, false, DUAL, 4, Q8Out>(aa.a, FixedW<CIN / 64>{}, FixedW<COUT / 64>{}, aa.q);
}
template <int KW, bool PRE, bool ACT, bool DUAL>
__global__ void __launch_bounds__(256, 2) k_lconv_q8_any(LConvQAnyArgs aa) {
  lconv_body<KW, PRE, ACT, false, DUAL, 4, Q8Out>(aa.a, RuntimeW{aa.nip}, RuntimeW{aa.ncp}, aa.q);
}

template <int KW, int CIN, int COUT, bool ACT, bool RES, bool DUAL>
__global__ void __launch_bounds__(kWgI8, 2) k_lconv_i8_f16(LConvI8Args a) {
  lconv_i8_body<KW, FixedW<CIN>, FixedW<COUT>, false, ACT, RES, DUAL, true>(a, FixedW<CIN>{}, FixedW<COUT>{});
}
template <int KW, bool ACT, bool RES, bool DUAL>
__global__ void __launch_bounds__(kWgI8, 2) k_lconv_i8_f16_any(LConvI8Args a, int cin, int cout) {
  lconv_i8_body<KW, RuntimeW, RuntimeW, false, ACT, RES, DUAL, true>(a, RuntimeW{cin}, RuntimeW{cout});
}

// the launch of launch_lconv_nw (kernels.hip) / launch_lconv_t (conv_any.hip), 4-wave form
template <int KW, bool PRE, bool ACT, bool DUAL>
hipError_t launch_q8_t(bool any, const LConvArgs& a, const Q8Out& q, int cin, int cout, int n_cu, hipStream_t s) {
  using G = Geo<1, 64, KW, 4, KW == 3 ? 2 : kKMS>;
  const int grid = conv_split_grid(a.npos, 1, cout / 64, 2 * n_cu);   // two workgroups per CU
  constexpr size_t lds = G::ACT_BYTES + ring_bytes(64, G::KMS);
  static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
  LConvArgs b = a;
  b.nms_total = a.nms_total * (kKMS / G::KMS);   // the host counts macro-steps of kKMS k16-steps
  static const bool turns = getenv("P3HIP_NO_PAIR_TURNS") == nullptr;
  b.pair_split = (turns && grid > n_cu) ? n_cu : 0;
  static AttrOnce once[2];
  if (any) {
    if (hipError_t e = ensure_lds(once[0], k_lconv_q8_any<KW, PRE, ACT, DUAL>, lds); e != hipSuccess) return e;
    const LConvQAnyArgs k{b, q, cin / 64, cout / 64};
    hipLaunchKernelGGL((k_lconv_q8_any<KW, PRE, ACT, DUAL>), dim3(grid), dim3(256), lds, s, k);
  } else {
    if (cin != 384 || cout != 192) return hipErrorInvalidValue;
    if (hipError_t e = ensure_lds(once[1], k_lconv_q8<KW, 384, 192, PRE, ACT, DUAL>, lds); e != hipSuccess) return e;
    const LConvQArgs k{b, q};
    hipLaunchKernelGGL((k_lconv_q8<KW, 384, 192, PRE, ACT, DUAL>), dim3(grid), dim3(256), lds, s, k);
  }
  return hipGetLastError();
}

template <int KW, bool ACT, bool RES, bool DUAL>
hipError_t launch_f16_t(bool any, int cin, int cout, const LConvI8Args& a, hipStream_t s) {
  constexpr size_t lds = 2 * kSliceBytes;
  static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
  const dim3 grid(a.npos * (cout / 64));
  if (any) {
    hipLaunchKernelGGL((k_lconv_i8_f16_any<KW, ACT, RES, DUAL>), grid, dim3(kWgI8), lds, s, a, cin, cout);
  } else {
    if (cin != 192 || cout != 192) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_lconv_i8_f16<KW, 192, 192, ACT, RES, DUAL>), grid, dim3(kWgI8), lds, s, a);
  }
  return hipGetLastError();
}

bool width_ok(int c) { return c >= 64 && c <= 512 && c % 64 == 0; }

}  // namespace

hipError_t launch_lconv_q8(bool any, int kw, int cin, int cout, const LConvArgs& a, const float* act_scale, int out_scale,
                           int n_cu, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  if (kw != 1 || !width_ok(cin) || !width_ok(cout) || a.res || (a.act != 0) == (a.dual != 0) || !act_scale || out_scale < 0)
    return hipErrorInvalidValue;
  const Q8Out q{act_scale, out_scale};
  if (a.act) return a.pre ? launch_q8_t<1, true, true, false>(any, a, q, cin, cout, n_cu, s)      // btl reduce from the raw stream
                          : launch_q8_t<1, false, true, false>(any, a, q, cin, cout, n_cu, s);    // .. from the activated copy
  return a.pre ? launch_q8_t<1, true, false, true>(any, a, q, cin, cout, n_cu, s)                 // nbt reduce (t raw + q(act1(t)))
               : launch_q8_t<1, false, false, true>(any, a, q, cin, cout, n_cu, s);
}

hipError_t launch_lconv_i8_f16(bool any, int kw, int cin, int cout, const LConvI8Args& a, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  if (kw != 3 || !width_ok(cin) || !width_ok(cout) || a.pre) return hipErrorInvalidValue;
  if (a.act && !a.res && !a.dual) return launch_f16_t<3, true, false, false>(any, cin, cout, a, s);   // the last inner conv of a btl block
  if (!a.act && a.res && a.dual) return launch_f16_t<3, false, true, true>(any, cin, cout, a, s);     // conv4 of an nbt block
  return hipErrorInvalidValue;
}

}  // namespace p3
