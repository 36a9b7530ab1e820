// transformer_split.h — the low-latency plan of the transformer trunks (include/p3hip.h P3HIP_FLAG_LOW_LATENCY_TFM):
// the three launches of a block (transformer.h) handed to more workgroups, for runs of a few positions that would
// otherwise occupy npos x heads CUs (attention) and npos x 361 / 64 CUs (qkv, ffn).  The attention of a (position, head)
// is split into S parts of its 23 query tiles; qkv and ffn take T = 16 or 32 tokens per workgroup instead of 64.  Every
// query row and every token row is computed independently of its neighbours, by the same chain of operations whatever
// (S, T): the split never changes a bit of the result, and the plan returns the bits of the default fp16 plan.
#pragma once
#include <hip/hip_runtime.h>

#include "transformer.h"

namespace p3 {

constexpr int kTfmQTiles = (kTfmL + 15) / 16;   // 23 query tiles of 16

// ---- the split ---------------------------------------------------------------------------------------
inline bool tfm_split_valid(int parts, int tokens) {
  return (parts == 1 || parts == 2 || parts == 3 || parts == 6) && (tokens == 16 || tokens == 32 || tokens == 64);
}

// The split of a launch over npos positions of a trunk with `heads` heads on n_cu CUs.  S, the query parts of the
// attention: the largest of {1, 2, 3, 6} whose npos x heads x S workgroups fit one round of the CUs (every part stages
// the whole K and V of its head, so a second round costs what the finer split saved), else 1.  T, the tokens per
// workgroup of qkv and ffn: the smallest of {16, 32, 64} whose ceil(npos x 361 / T) workgroups fit one round, else 64.
// More positions never give a finer split, and where it is (1, 64) the launches are those of the default plan.
inline void tfm_split(int npos, int heads, int n_cu, int* parts, int* tokens) {
  static const int kParts[3] = {6, 3, 2}, kTokens[2] = {16, 32};
  *parts = 1;
  for (int s : kParts)
    if ((long)npos * heads * s <= n_cu) { *parts = s; break; }
  *tokens = 64;
  for (int t : kTokens)
    if (((long)npos * kTfmL + t - 1) / t <= n_cu) { *tokens = t; break; }
}

// The launches of a block under the split.  parts = 1 is launch_tfm_attn and tokens = 64 launch_tfm_qkv / launch_tfm_ffn
// themselves (transformer.hip); anything outside tfm_split_valid returns hipErrorInvalidValue.
hipError_t launch_tfm_qkv_split(int C, int D, const TfmQkvArgs& a, int tokens, hipStream_t s);
hipError_t launch_tfm_attn_split(int D, const TfmAttnArgs& a, int parts, hipStream_t s);
hipError_t launch_tfm_ffn_split(int C, const TfmFfnArgs& a, int tokens, hipStream_t s);

}  // namespace p3
