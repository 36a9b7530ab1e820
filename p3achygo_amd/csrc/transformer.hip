// transformer.hip — the transformer trunk (python/model_transformer.py TransformerBlock) on v_mfma_f32_16x16x32_f16,
// for every model width C and head width D of the supported set (transformer.h tfm_supported).  Three launches per block:
//   k_tfm_qkv<C, D>  64 tokens per workgroup: RMSNorm_in, x^ . [Wq | Wk | Wv], spiral RoPE on q and k  -> q, k, v fp16
//   k_tfm_attn<D>    one workgroup per (position, head): K and V in LDS, full-row softmax over the 361 keys  -> o fp16
//   k_tfm_ffn<C>     64 tokens per workgroup: o . Wo + x, RMSNorm_out, silu(x^ . Wgate) * (x^ . Wup), . Wdown + residual
// The kernel bodies are transformer_{qkv,attn,ffn}_body.inc, the text transformer_split.hip's kernels are made of too,
// here at NT = 4 token tiles of 16 per workgroup and over all 23 query tiles; transformer_core.h has the layouts, the
// number formats and why the bodies are included as text.
#include "transformer.h"

#include "transformer_core.h"

namespace p3 {
namespace {

template <int C, int D>
__global__ __launch_bounds__(256) void k_tfm_qkv(TfmQkvArgs a) {
  constexpr int NT = 4;
#include "transformer_qkv_body.inc"
}

// one workgroup per (position, head) = blockIdx.x, all 23 query tiles
template <int D>
__global__ __launch_bounds__(256) void k_tfm_attn(TfmAttnArgs a) {
  const int nh = a.heads;
  const int p = blockIdx.x / nh, head = blockIdx.x % nh;
  constexpr int qt0 = 0, q1 = kTfmL;
#include "transformer_attn_body.inc"
}

template <int C>
__global__ __launch_bounds__(256) void k_tfm_ffn(TfmFfnArgs a) {
  constexpr int NT = 4;
#include "transformer_ffn_body.inc"
}

}  // namespace

hipError_t launch_tfm_qkv(int C, int D, const TfmQkvArgs& a, hipStream_t s) {
  if (D < 1 || !tfm_supported(C, C / D)) return hipErrorInvalidValue;
  return dispatch_c(C, [&](auto c) {
    constexpr int kC = decltype(c)::value;
    if (D == 32) hipLaunchKernelGGL((k_tfm_qkv<kC, 32>), dim3(token_tiles(a.npos, 64)), dim3(256), 0, s, a);
    else if constexpr (kC % 64 == 0) hipLaunchKernelGGL((k_tfm_qkv<kC, 64>), dim3(token_tiles(a.npos, 64)), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}
hipError_t launch_tfm_attn(int D, const TfmAttnArgs& a, hipStream_t s) {
  if (D == 32) hipLaunchKernelGGL(k_tfm_attn<32>, dim3(a.npos * a.heads), dim3(256), 0, s, a);
  else if (D == 64) hipLaunchKernelGGL(k_tfm_attn<64>, dim3(a.npos * a.heads), dim3(256), 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t launch_tfm_ffn(int C, const TfmFfnArgs& a, hipStream_t s) {
  return dispatch_c(C, [&](auto c) {
    hipLaunchKernelGGL((k_tfm_ffn<decltype(c)::value>), dim3(token_tiles(a.npos, 64)), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace p3
