// transformer_split.hip — the transformer block's three launches for runs of a few positions (transformer_split.h,
// P3HIP_FLAG_LOW_LATENCY_TFM), for gfx950, on v_mfma_f32_16x16x32_f16:
//   k_tfm_qkv_split<C, D, NT>  16 NT tokens per workgroup (NT = 1, 2) instead of 64
//   k_tfm_attn_split<D>        one workgroup per (position, head, part): K and V^T of the head in LDS as k_tfm_attn stages
//                              them, and the 16-query step on the part's share of the 23 query tiles only
//   k_tfm_ffn_split<C, NT>     16 NT tokens per workgroup
// The kernel bodies are transformer_{qkv,attn,ffn}_body.inc, the text transformer.hip's kernels are made of, at another
// token-tile count and over a part of the query tiles: one text, so per token and per query the same operations (and
// transformer.hip's kernels, symbols and registers stay as they are: transformer_core.h).
// tests/test_low_latency_tfm_gpu.py holds the two plans to equal bytes.
#include "transformer_split.h"

#include "transformer_core.h"

namespace p3 {
namespace {

template <int C, int D, int NT>
__global__ __launch_bounds__(256) void k_tfm_qkv_split(TfmQkvArgs a) {
#include "transformer_qkv_body.inc"
}

// One (position, head, part) per workgroup: blockIdx.x = (position x heads + head) x parts + part.  The part's query tiles
// are the ceil(23 / parts) from part x ceil(23 / parts) on (12 + 11, 8 + 8 + 7, 5 x 4 + 3), a wave takes every fourth (at
// 6 parts one tile per wave: the last part has 3, and its last tile the queries 352 .. 360 and seven masked ones).  Every
// query 0 .. 360 belongs to exactly one part.
template <int D>
__global__ __launch_bounds__(256) void k_tfm_attn_split(TfmAttnArgs a, int parts) {
  const int nh = a.heads;
  const int ph = blockIdx.x / parts, part = blockIdx.x - ph * parts;
  const int p = ph / nh, head = ph % nh;
  const int per = (kTfmQTiles + parts - 1) / parts;
  const int qt0 = part * per, q1 = 16 * min(qt0 + per, kTfmQTiles);
#include "transformer_attn_body.inc"
}

template <int C, int NT>
__global__ __launch_bounds__(256) void k_tfm_ffn_split(TfmFfnArgs a) {
#include "transformer_ffn_body.inc"
}

}  // namespace

hipError_t launch_tfm_qkv_split(int C, int D, const TfmQkvArgs& a, int tokens, hipStream_t s) {
  if (!tfm_split_valid(1, tokens) || D < 1 || !tfm_supported(C, C / D)) return hipErrorInvalidValue;
  if (tokens == 64) return launch_tfm_qkv(C, D, a, s);
  const dim3 grid(token_tiles(a.npos, tokens));
  return dispatch_c(C, [&](auto c) {
    constexpr int kC = decltype(c)::value;
    if (D == 32) {
      if (tokens == 16) hipLaunchKernelGGL((k_tfm_qkv_split<kC, 32, 1>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_tfm_qkv_split<kC, 32, 2>), grid, dim3(256), 0, s, a);
    } else if constexpr (kC % 64 == 0) {
      if (tokens == 16) hipLaunchKernelGGL((k_tfm_qkv_split<kC, 64, 1>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_tfm_qkv_split<kC, 64, 2>), grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
  });
}

hipError_t launch_tfm_attn_split(int D, const TfmAttnArgs& a, int parts, hipStream_t s) {
  if (!tfm_split_valid(parts, 64)) return hipErrorInvalidValue;
  if (parts == 1) return launch_tfm_attn(D, a, s);
  const dim3 grid(a.npos * a.heads * parts);
  if (D == 32) hipLaunchKernelGGL(k_tfm_attn_split<32>, grid, dim3(256), 0, s, a, parts);
  else if (D == 64) hipLaunchKernelGGL(k_tfm_attn_split<64>, grid, dim3(256), 0, s, a, parts);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_tfm_ffn_split(int C, const TfmFfnArgs& a, int tokens, hipStream_t s) {
  if (!tfm_split_valid(1, tokens)) return hipErrorInvalidValue;
  if (tokens == 64) return launch_tfm_ffn(C, a, s);
  const dim3 grid(token_tiles(a.npos, tokens));
  return dispatch_c(C, [&](auto c) {
    constexpr int kC = decltype(c)::value;
    if (tokens == 16) hipLaunchKernelGGL((k_tfm_ffn_split<kC, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_tfm_ffn_split<kC, 2>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace p3
