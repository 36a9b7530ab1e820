// loss.h — the trainer's validation-loss terms of every output row that has targets, on the device (include/p3hip.h,
// "the trainer's validation losses"; python/model.py:1297-1572).  Kernels in loss.hip, the ABI in loss_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/p3hip.h"

namespace p3 {

// The device copy of a p3hip_targets: every array starts on a 16-byte boundary (the struct's do not: 362 floats), padded
// with zeros, so that a wave reads a target vector with the same float4 loads as the logits it is paired with.
constexpr int kTgtPolicy = 0;       // 362 (+2)
constexpr int kTgtAuxDist = 364;    // 362 (+2)
constexpr int kTgtOwn = 728;        // 361 (+3)
constexpr int kTgtMcts = 1092;      // 51 (+1)
constexpr int kTgtScalars = 1144;   // score_margin, q6, q16, q50, q6_score, q16_score, q50_score
constexpr int kTgtInts = 1151;      // policy_aux, has_pi_aux_dist, has_mcts_value_dist (int bits)
constexpr int kTgtStride = 1156;
static_assert(kTgtStride % 4 == 0 && kTgtAuxDist % 4 == 0 && kTgtOwn % 4 == 0 && kTgtMcts % 4 == 0, "16-byte aligned arrays");

inline void pack_targets(const p3hip_targets& t, float* d) {
  std::memset(d, 0, kTgtStride * sizeof(float));
  std::memcpy(d + kTgtPolicy, t.policy, sizeof t.policy);
  std::memcpy(d + kTgtAuxDist, t.policy_aux_dist, sizeof t.policy_aux_dist);
  std::memcpy(d + kTgtOwn, t.own, sizeof t.own);
  std::memcpy(d + kTgtMcts, t.mcts_value_dist, sizeof t.mcts_value_dist);
  std::memcpy(d + kTgtScalars, &t.score_margin, 7 * sizeof(float));
  std::memcpy(d + kTgtInts, &t.policy_aux, 3 * sizeof(int32_t));
}

struct LossArgs {
  const float* out;       // [..][kOutStride]: the rows the heads wrote
  const float* aux;       // [..][kAuxStride]: the records k_heads_aux wrote
  const int* rows;        // [n] row of `out` and `aux` that entry k belongs to
  const float* targets;   // [n][kTgtStride]
  float* terms;           // [n][P3HIP_NUM_LOSS_TERMS]
  double* sums;           // [P3HIP_NUM_LOSS_TERMS]
  int n;
};
// k_loss_rows (one workgroup per entry) then k_loss_sum (one workgroup) on stream s
hipError_t launch_loss(const LossArgs& a, hipStream_t s);

}  // namespace p3
