// loss.hip — the 19 validation-loss terms of every output row that has targets, and their sums (loss.h; the definitions
// are in include/p3hip.h, "the trainer's validation losses", with the lines of python/model.py they restate).
//
// One workgroup of six waves per entry; every wave owns whole vectors, so no value crosses a wave and the kernel has no
// barrier and no LDS: wave 0 pi_logits, 1 pi_logits_optimistic, 2 pi_logits_aux, 3 pi_logits_soft (one 362-wide
// log-sum-exp and clipped KLD each), 4 the 800 score logits (softmax, prefix sum, squared CDF distance), 5 ownership, the
// 51 mcts bins and the scalar heads.  A wave reads its vector once into registers: 16-byte loads where the vector starts
// on a 16-byte boundary (pi_logits, pi_logits_aux and the targets paired with them, loss.h), 4-byte loads elsewhere
// (the other vectors of an output row start at odd float offsets).  About 18 KB are read per entry (the policy target three times, by the three waves that use it).
//
// The arithmetic is double, every term rounded to float once (include/p3hip.h): some 4,000 exp / log per entry, which
// at batch 1024 is noise beside the forward pass, and it keeps each term within a rounding of the float64 restatement
// whatever order the wave adds in.  Wave reductions are xor butterflies in a fixed order: ds_swizzle within 32 lanes,
// one ds_bpermute across the halves.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "heads_aux.h"
#include "kernels.h"
#include "loss.h"

namespace p3 {
namespace {

constexpr int kWave = 64;
constexpr int kWaves = 6;
constexpr int kSumThreads = 256;
constexpr int kTerms = P3HIP_NUM_LOSS_TERMS;
constexpr int kMoves = P3HIP_NUM_MOVES;
constexpr int kBins = P3HIP_NUM_SCORE_LOGITS;
constexpr int kBinsPerLane = 13;   // 64 x 13 = 832 >= 800: lane l owns bins 13 l .. 13 l + 12
static_assert(kWave * kBinsPerLane >= kBins, "every score bin has a lane");
constexpr double kEps = (double)1e-7f;     // keras.backend.epsilon() as the float32 graph holds it
constexpr double kZEps = (double)1e-6f;    // model.py:1460

// ---- cross-lane ------------------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ int lane_xor_i(int v) {
  if constexpr (D < 32) return __builtin_amdgcn_ds_swizzle(v, (D << 10) | 0x1f);   // bit mode: and 0x1f, or 0, xor D
  else return __shfl_xor(v, 32, kWave);
}
template <int D>
__device__ __forceinline__ double lane_xor(double v) {
  return __hiloint2double(lane_xor_i<D>(__double2hiint(v)), lane_xor_i<D>(__double2loint(v)));
}
__device__ __forceinline__ double wave_sum(double v) {
  v += lane_xor<1>(v); v += lane_xor<2>(v); v += lane_xor<4>(v);
  v += lane_xor<8>(v); v += lane_xor<16>(v); v += lane_xor<32>(v);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, lane_xor<1>(v)); v = fmax(v, lane_xor<2>(v)); v = fmax(v, lane_xor<4>(v));
  v = fmax(v, lane_xor<8>(v)); v = fmax(v, lane_xor<16>(v)); v = fmax(v, lane_xor<32>(v));
  return v;
}
// (value, index) of the wave's first maximum: the larger value wins, the lower index among equal values
template <int D>
__device__ __forceinline__ void argmax_step(float& best, int& bi) {
  const float ov = __int_as_float(lane_xor_i<D>(__float_as_int(best)));
  const int oi = lane_xor_i<D>(bi);
  if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
}

// ---- a 362-wide vector in a wave's registers ----------------------------------------------------------------------------
// V4: lane l holds elements 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3 (two float4 loads; the second for l <= 26, whose
// last piece covers 360 .. 363: every 16-byte aligned 362-vector here has at least two readable floats behind it).
// Otherwise lane l holds l, l + 64, ...  A logit vector and the target it is paired with use the same layout.
template <bool V4>
struct Vec {
  static constexpr int N = V4 ? 8 : 6;
  static __device__ __forceinline__ int idx(int lane, int j) {
    return V4 ? (j < 4 ? 4 * lane + j : 256 + 4 * lane + (j - 4)) : lane + kWave * j;
  }
  static __device__ __forceinline__ void load(const float* p, int lane, float (&v)[N]) {
    if constexpr (V4) {
      const float4 a = *reinterpret_cast<const float4*>(p + 4 * lane);
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane <= 26) b = *reinterpret_cast<const float4*>(p + 256 + 4 * lane);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) v[j] = idx(lane, j) < kMoves ? p[idx(lane, j)] : 0.f;
    }
  }
};

struct Lse { double m, sum; };   // max and sum exp(x - m): log_softmax(x)_i = x_i - m - log(sum)

template <bool V4>
__device__ __forceinline__ Lse lse362(const float (&x)[Vec<V4>::N], int lane) {
  double m = -INFINITY;
#pragma unroll
  for (int j = 0; j < Vec<V4>::N; ++j)
    if (Vec<V4>::idx(lane, j) < kMoves) m = fmax(m, (double)x[j]);
  m = wave_max(m);
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < Vec<V4>::N; ++j)
    if (Vec<V4>::idx(lane, j) < kMoves) s += exp((double)x[j] - m);
  return Lse{m, wave_sum(s)};
}

__device__ __forceinline__ double clip_eps(double v) { return fmin(fmax(v, kEps), 1.0); }
// one element of keras.metrics.kl_divergence(t, p)
__device__ __forceinline__ double kld_term(double t, double p) {
  const double tc = clip_eps(t), pc = clip_eps(p);
  return tc * log(tc / pc);
}

// KLD(t * scale, softmax(x)) over the 362 entries; every lane returns it
template <bool V4>
__device__ __forceinline__ double kld362(const float (&x)[Vec<V4>::N], const double (&t)[Vec<V4>::N], const Lse& l, int lane) {
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < Vec<V4>::N; ++j)
    if (Vec<V4>::idx(lane, j) < kMoves) acc += kld_term(t[j], exp((double)x[j] - l.m) / l.sum);
  return wave_sum(acc);
}

// first maximum of the 362 entries (numpy / keras argmax on finite values): every lane returns the index
template <bool V4>
__device__ __forceinline__ int argmax362(const float (&x)[Vec<V4>::N], int lane) {
  float best = -INFINITY;
  int bi = INT_MAX;
#pragma unroll
  for (int j = 0; j < Vec<V4>::N; ++j) {
    const int i = Vec<V4>::idx(lane, j);
    if (i < kMoves && (x[j] > best || (x[j] == best && i < bi))) { best = x[j]; bi = i; }
  }
  argmax_step<1>(best, bi); argmax_step<2>(best, bi); argmax_step<4>(best, bi);
  argmax_step<8>(best, bi); argmax_step<16>(best, bi); argmax_step<32>(best, bi);
  return bi == INT_MAX ? 0 : bi;
}

__device__ __forceinline__ double huber(double y_true, double y_pred) {   // keras.losses.Huber(), delta 1
  const double e = fabs(y_pred - y_true);
  return e <= 1.0 ? 0.5 * e * e : e - 0.5;
}
__device__ __forceinline__ double sq(double v) { return v * v; }

template <bool V4>
__device__ __forceinline__ void to_double(const float (&t)[Vec<V4>::N], double (&d)[Vec<V4>::N]) {
#pragma unroll
  for (int j = 0; j < Vec<V4>::N; ++j) d[j] = (double)t[j];
}

__global__ __launch_bounds__(kWave * kWaves) void k_loss_rows(LossArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k = blockIdx.x;
  if (k >= a.n) return;
  const int row = a.rows[k];
  const float* r = a.out + (size_t)row * kOutStride;
  const float* x = a.aux + (size_t)row * kAuxStride;
  const float* t = a.targets + (size_t)k * kTgtStride;
  float* o = a.terms + (size_t)k * kTerms;
  const float margin = t[kTgtScalars];

  if (wave == 0) {          // [0] policy, [17] move_hit
    float lg[8], tg[8];
    double td[8];
    Vec<true>::load(r + kOffMoveLogits, lane, lg);
    Vec<true>::load(t + kTgtPolicy, lane, tg);
    to_double<true>(tg, td);
    const Lse l = lse362<true>(lg, lane);
    const double kld = kld362<true>(lg, td, l, lane);
    const int hit = argmax362<true>(lg, lane) == argmax362<true>(tg, lane);
    if (lane == 0) { o[0] = (float)kld; o[17] = hit ? 1.0f : 0.0f; }
  } else if (wave == 1) {   // [15] pi_optimistic
    float lg[6], tg[6];
    double td[6];
    Vec<false>::load(r + kOffOptLogits, lane, lg);
    Vec<false>::load(t + kTgtPolicy, lane, tg);
    to_double<false>(tg, td);
    const Lse l = lse362<false>(lg, lane);
    const double kld = kld362<false>(lg, td, l, lane);
    const double z6 = ((double)t[kTgtScalars + 1] - (double)x[kAuxOffQ + 0]) / sqrt((double)r[kOffErr2] + kZEps);
    const double z16 = ((double)t[kTgtScalars + 2] - (double)x[kAuxOffQ + 1]) / sqrt((double)x[kAuxOffQErr + 0] + kZEps);
    const double z50 = ((double)t[kTgtScalars + 3] - (double)x[kAuxOffQ + 2]) / sqrt((double)x[kAuxOffQErr + 1] + kZEps);
    const double decay = 4.0 / 7.0;
    const double z = (decay * 3 * z6 + decay * 1.5 * z16 + decay * 0.75 * z50) / 3.0;
    const double w = fmin(fmax(1.0 / (1.0 + exp(-(z - 1.0) * 3)), 0.0), 1.0);
    if (lane == 0) o[15] = (float)(kld * w);
  } else if (wave == 2) {   // [1] policy_aux_dist, [2] policy_aux_scalar
    float lg[8], tg[8];
    double td[8];
    Vec<true>::load(x + kAuxOffPiAux, lane, lg);
    Vec<true>::load(t + kTgtAuxDist, lane, tg);
    to_double<true>(tg, td);
    const Lse l = lse362<true>(lg, lane);
    const double kld = kld362<true>(lg, td, l, lane);
    const int* ti = reinterpret_cast<const int*>(t + kTgtInts);
    const int pa = min(max(ti[0], 0), kMoves - 1);   // (p3hip_load_targets refuses anything else)
    const double has = ti[1] != 0 ? 1.0 : 0.0;
    const double scce = fmin(fmax(log(l.sum) + l.m - (double)x[kAuxOffPiAux + pa], 0.0), 50.0);
    if (lane == 0) { o[1] = (float)(has * kld); o[2] = (float)((1.0 - has) * scce); }
  } else if (wave == 3) {   // [14] pi_soft
    float lg[6], tg[6];
    double td[6];
    Vec<false>::load(x + kAuxOffPiSoft, lane, lg);
    Vec<false>::load(t + kTgtPolicy, lane, tg);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      td[j] = Vec<false>::idx(lane, j) < kMoves ? pow((double)tg[j], 0.25) : 0.0;
      s += td[j];
    }
    s = wave_sum(s);
#pragma unroll
    for (int j = 0; j < 6; ++j) td[j] /= s;
    const Lse l = lse362<false>(lg, lane);
    const double kld = kld362<false>(lg, td, l, lane);
    if (lane == 0) o[14] = (float)kld;
  } else if (wave == 4) {   // [7] score_pdf, [8] score_cdf
    const float* sl = r + kOffScoreLogits;
    const int b0 = lane * kBinsPerLane;
    float v[kBinsPerLane];
    double m = -INFINITY;
#pragma unroll
    for (int j = 0; j < kBinsPerLane; ++j) {
      v[j] = b0 + j < kBins ? sl[b0 + j] : -INFINITY;
      m = fmax(m, (double)v[j]);
    }
    m = wave_max(m);
    double e[kBinsPerLane], mine = 0.0;
#pragma unroll
    for (int j = 0; j < kBinsPerLane; ++j) {
      e[j] = b0 + j < kBins ? exp((double)v[j] - m) : 0.0;
      mine += e[j];
    }
    // inclusive scan of the lanes' sums (Hillis-Steele), then this lane's bins continue from the lanes in front of it
    double incl = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const double up = __shfl_up(incl, d, kWave);
      if (lane >= d) incl += up;
    }
    const double total = __shfl(incl, kWave - 1, kWave);
    const double kd = floor((double)margin) + 400.0;   // transforms.py:246-251
    const int kk = kd < 0.0 ? 0 : kd > (double)(kBins - 1) ? kBins - 1 : (int)kd;
    double run = incl - mine, acc = 0.0;
#pragma unroll
    for (int j = 0; j < kBinsPerLane; ++j) {
      run += e[j];
      if (b0 + j < kBins) acc += sq((b0 + j >= kk ? 1.0 : 0.0) - run / total);
    }
    acc = wave_sum(acc);
    const double pdf = log(total) + m - (double)sl[kk];
    if (lane == 0) { o[7] = (float)pdf; o[8] = (float)acc; }
  } else {                  // [3] outcome, [4..6] q, [9] own, [10] gamma_sq, [11..13] the q heads, [16] mcts_dist, [18] outcome_hit
    double own = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int i = lane + kWave * j;
      if (i < P3HIP_NUM_LOCS) own += sq((double)t[kTgtOwn + i] - (double)r[kOffOwnership + i]);
    }
    own = wave_sum(own) / (double)P3HIP_NUM_LOCS;
    const bool bin = lane < kAuxBins;
    const double cnt = bin ? (double)t[kTgtMcts + lane] : 0.0;
    const double ml = bin ? (double)x[kAuxOffMctsLogits + lane] : -INFINITY;
    const double total = fmax(wave_sum(cnt), 1.0);
    const double mm = wave_max(ml);
    const double me = bin ? exp(ml - mm) : 0.0;
    const double ms = wave_sum(me);
    const double mk = wave_sum(bin ? kld_term(cnt / total, me / ms) : 0.0);
    if (lane == 0) {
      const int* ti = reinterpret_cast<const int*>(t + kTgtInts);
      const double l0 = r[kOffOutcomeLogits], l1 = r[kOffOutcomeLogits + 1];
      const double om = fmax(l0, l1), ol = om + log(exp(l0 - om) + exp(l1 - om));
      const double g1 = margin > 0.0f ? 1.0 : margin < 0.0f ? 0.0 : 0.5;
      o[3] = (float)(-((1.0 - g1) * (l0 - ol) + g1 * (l1 - ol)));
      double qe = 0.0, qs = 0.0, qse = 0.0;
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const double q = t[kTgtScalars + 1 + h], qp = x[kAuxOffQ + h];
        const double err = h == 0 ? (double)r[kOffErr2] : (double)x[kAuxOffQErr + h - 1];
        const double s = t[kTgtScalars + 4 + h], sp = x[kAuxOffQScore + h], se = x[kAuxOffQScoreErr + h];
        o[4 + h] = (float)sq(q - qp);
        qe += huber(sq(qp - q), err);
        qs += huber(s / 10.0, sp / 10.0);
        qse += huber(sq(sp - s) / 100.0, se / 100.0);
      }
      o[9] = (float)own;
      o[10] = (float)sq((double)r[kOffGamma]);
      o[11] = (float)(qe / 3.0);
      o[12] = (float)(qs / 3.0);
      o[13] = (float)(qse / 3.0);
      o[16] = (float)((ti[2] != 0 ? 1.0 : 0.0) * mk);
      o[18] = ((l1 > l0) == (margin >= 0.0f)) ? 1.0f : 0.0f;
    }
  }
}

// One workgroup, a fixed order (k_score_sum's): thread t adds entries t, t + 256, ... in ascending order, in double; then
// a binary tree over the 256 partial sums in LDS.  The order depends on n alone: the same terms always give the same bits.
__global__ __launch_bounds__(kSumThreads) void k_loss_sum(LossArgs a) {
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

hipError_t launch_loss(const LossArgs& a, hipStream_t s) {
  if (a.n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_loss_rows, dim3(a.n), dim3(kWave * kWaves), 0, s, a);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(k_loss_sum, dim3(1), dim3(kSumThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace p3
