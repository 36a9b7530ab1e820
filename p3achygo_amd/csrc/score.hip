// score.hip — the six DefaultStats terms of every labelled output row, and their sums (score.h).
//
// About 6 KB are read per position (362 + 2 + 800 probabilities and a 1,456 B label): the point is not speed of the
// kernel but that a scoring run moves 24 bytes per position to the host instead of a 7.5 KB result record.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "kernels.h"
#include "score.h"

namespace p3 {
namespace {

constexpr int kWave = 64;
constexpr int kRowsPerWg = 4;    // k_score_rows: four waves, one entry each
constexpr int kSumThreads = 256;
constexpr int kTerms = P3HIP_NUM_SCORE_TERMS;

// Argmax of benchmark_engine.cc:11-22 over v[0 .. n): a sequential scan from (-FLT_MAX, index 0) that advances on
// strict >, so the lowest index among the largest non-NaN values above -FLT_MAX, or 0 when there is none.  A lane scans
// its indices lane, lane + 64, ... in ascending order with the same strict > (its lowest index of its largest value;
// INT_MAX: nothing above -FLT_MAX yet), then the wave reduces over (value, index): the larger value wins, the lower
// index among equal values.  Every lane returns the result.
__device__ inline int wave_argmax(const float* v, int n, int lane) {
  float best = -FLT_MAX;
  int bi = INT_MAX;
  for (int i = lane; i < n; i += kWave) {
    const float x = v[i];
    if (x > best) { best = x; bi = i; }   // false for NaN
  }
#pragma unroll
  for (int d = kWave / 2; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(best, d, kWave);
    const int oi = __shfl_xor(bi, d, kWave);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  return bi == INT_MAX ? 0 : bi;
}

// -std::log(p), or kMaxLoss = 16 when p == 0 (benchmark_engine.cc:27,37-43; -0.0 counts as 0).  The logarithm is taken in
// double and rounded once: within 0.5 ulp of the exact value, as the host's logf is to all intents.  The device's logf was
// measured up to 2.08 fp32 ulp away on an MI355X; two logarithms per position cost nothing.
__device__ inline float ce_loss(float p) { return p != 0.0f ? (float)-log((double)p) : 16.0f; }

__global__ __launch_bounds__(kWave * kRowsPerWg) void k_score_rows(ScoreArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int k = blockIdx.x * kRowsPerWg + (threadIdx.x >> 6);
  if (k >= a.n) return;   // whole waves leave: no barrier below
  const float* r = a.out + (size_t)a.rows[k] * kOutStride;
  const p3hip_labels* lab = a.labels + k;
  const int mv_pred = wave_argmax(r + kOffMoveProbs, P3HIP_NUM_MOVES, lane);
  const int outcome_pred = wave_argmax(r + kOffValueProbs, P3HIP_NUM_VALUE_LOGITS, lane);
  const int score_arg = wave_argmax(r + kOffScoreProbs, P3HIP_NUM_SCORE_LOGITS, lane);
  const int mv = wave_argmax(lab->policy, P3HIP_NUM_MOVES, lane);
  const int did_win = lab->did_win != 0;
  // `int score_pred = Argmax(score_probs) + 0.5 - kScoreInflectionPoint` (benchmark_engine.cc:30-31): the double is
  // truncated toward zero, so bins 399 and 400 both predict 0
  const int score_pred = (int)((double)score_arg + 0.5 - 400.0);
  float t = 0.0f;
  switch (lane) {
    case 0: t = ce_loss(r[kOffMoveProbs + mv]); break;
    case 1: t = ce_loss(r[kOffValueProbs + did_win]); break;
    case 2: t = mv == mv_pred ? 1.0f : 0.0f; break;
    case 3: t = did_win == outcome_pred ? 1.0f : 0.0f; break;
    case 4: t = fabsf(lab->score_margin - (float)score_pred); break;   // :59-60, float - int in float
    case 5: t = (float)score_pred; break;
  }
  if (lane < kTerms) a.terms[(size_t)k * kTerms + lane] = t;
}

// One workgroup, a fixed order: thread t adds entries t, t + 256, ... in ascending order, in double; then a binary tree
// over the 256 partial sums in LDS.  The order depends on n alone, so the same terms always give the same bits.
__global__ __launch_bounds__(kSumThreads) void k_score_sum(ScoreArgs a) {
  __shared__ double part[kTerms][kSumThreads];
  const int t = threadIdx.x;
  double acc[kTerms];
#pragma unroll
  for (int j = 0; j < kTerms; ++j) acc[j] = 0.0;
  for (int k = t; k < a.n; k += kSumThreads)
#pragma unroll
    for (int j = 0; j < kTerms; ++j) acc[j] += (double)a.terms[(size_t)k * kTerms + j];
#pragma unroll
  for (int j = 0; j < kTerms; ++j) part[j][t] = acc[j];
  __syncthreads();
  for (int half = kSumThreads / 2; half >= 1; half >>= 1) {
    if (t < half)
#pragma unroll
      for (int j = 0; j < kTerms; ++j) part[j][t] += part[j][t + half];
    __syncthreads();
  }
  if (t < kTerms) a.sums[t] = part[t][0];
}

}  // namespace

hipError_t launch_score(const ScoreArgs& a, hipStream_t s) {
  if (a.n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_score_rows, dim3((a.n + kRowsPerWg - 1) / kRowsPerWg), dim3(kWave * kRowsPerWg), 0, s, a);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(k_score_sum, dim3(1), dim3(kSumThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace p3
