// score.h — scoring the heads' output rows against labels on the device (include/p3hip.h, "scoring against labels";
// DefaultStats::Update, cc/nn/engine/benchmark_engine.cc:25-61).  Kernels in score.hip, the ABI in scoring.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/p3hip.h"

namespace p3 {

struct ScoreArgs {
  const float* out;             // [..][kOutStride]: the rows the heads (or k_sym_reduce, k_cache_fill) wrote
  const int* rows;              // [n] row of `out` that entry k scores
  const p3hip_labels* labels;   // [n] its labels
  float* terms;                 // [n][P3HIP_NUM_SCORE_TERMS]
  double* sums;                 // [P3HIP_NUM_SCORE_TERMS]
  int n;
};
// k_score_rows (one wave per entry) then k_score_sum (one workgroup) on stream s
hipError_t launch_score(const ScoreArgs& a, hipStream_t s);

}  // namespace p3
