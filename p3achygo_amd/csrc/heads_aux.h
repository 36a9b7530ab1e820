// heads_aux.h — k_heads_aux (heads_aux.hip): the fifteen outputs of the model the heads kernels leave out, one record per
// position (P3HIP_FLAG_AUX, include/p3hip.h p3hip_get_aux).
#pragma once
#include <hip/hip_runtime.h>

namespace p3 {

// Per-position fp32 record k_heads_aux writes; the first kAuxFloats are include/p3hip.h's P3HIP_AUX_LEN record, the rest of
// the 16-byte aligned row is zero.
constexpr int kAuxOffPiAux = 0;        // 362  08:pi_logits_aux (pass at 361)
constexpr int kAuxOffPiSoft = 362;     // 362  21:pi_logits_soft
constexpr int kAuxOffQ = 724;          // 3    09:q6 10:q16 11:q50          tanh(go[2..4])
constexpr int kAuxOffQErr = 727;       // 2    13:q16_err 14:q50_err        4 sigmoid(go[6..7])
constexpr int kAuxOffQScore = 729;     // 3    15..17:q*_score              go[8..10]
constexpr int kAuxOffQScoreErr = 732;  // 3    18..20:q*_score_err          |go[11..13]|
constexpr int kAuxOffMctsLogits = 735; // 51   23:mcts_dist_logits
constexpr int kAuxOffMctsProbs = 786;  // 51   24:mcts_dist_probs
constexpr int kAuxFloats = 837;
constexpr int kAuxStride = 840;
constexpr int kAuxBins = 51;           // model.py NUM_V_BUCKETS
constexpr int kAuxGoCols = 11;         // the columns of value.oq_out the heads kernels do not read: 2, 3, 4, 6 .. 13

struct HeadsAuxArgs {
  const float* hp;   // [npos][96 / 4][361][4]: the head convs' output, HeadsArgs::hp
  float* aux;        // [npos][kAuxStride]
  int npos;
  int V;
  // shared with the heads kernels (HeadsArgs)
  const float *gbn_scale, *gbn_shift;     // policy.gpool_bn folded [32]
  const float *gd_w, *gd_b;               // policy.gpool_dense [64][32], [32]
  const float *oq_embed_w, *oq_embed_b;   // [64][V], [V]
  // the aux tensors (plan.cpp kAuxTensors)
  const float* soft_moves_w;              // policy.soft_moves [32]
  const float *soft_pass_w, *soft_pass_b; // policy.soft_pass [64], [1]
  const float *mcts_w, *mcts_b;           // value.mcts_dist [V][51], [51]
  const float* moves_aux_w;               // column 1 of policy.out_moves [32]
  const float *pass_aux_w, *pass_aux_b;   // column 1 of policy.out_pass [64], [1]
  const float *oq_aux_w, *oq_aux_b;       // columns 2, 3, 4, 6 .. 13 of value.oq_out [V][11], [11]
};

hipError_t launch_heads_aux(const HeadsAuxArgs& a, int n_cu, hipStream_t s);

}  // namespace p3
