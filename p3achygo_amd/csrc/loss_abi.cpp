// loss_abi.cpp — the validation-loss entry points of the p3hip C ABI (include/p3hip.h, "the trainer's validation losses on
// the device"): targets per slot in pinned memory in the device layout of loss.h, gathered by output row, the terms
// computed by csrc/loss.hip on the engine's stream.  The twin of scoring.cpp, point for point.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "engine.h"
#include "loss.h"

using namespace eng;

namespace {

constexpr int kTerms = P3HIP_NUM_LOSS_TERMS;
static_assert(sizeof(p3hip_targets) == 4 * 1146, "p3hip_targets layout");
static_assert(offsetof(p3hip_targets, score_margin) == 4 * 1136 && offsetof(p3hip_targets, policy_aux) == 4 * 1143, "p3hip_targets layout");

// The loss buffers, made once.  p3hip_load_targets is called like p3hip_load_slot, from many threads at once.
bool ensure_loss(p3hip_engine* e) {
  auto& s = e->loss;
  if (s.ready.load(std::memory_order_acquire)) return true;
  std::lock_guard<std::mutex> lock(s.mu);
  if (s.ready.load(std::memory_order_relaxed)) return true;
  if (!e->bind()) return false;
  const size_t B = (size_t)e->batch, dense = B * p3::kTgtStride * sizeof(float);
  const bool ok = e->check(hipHostMalloc((void**)&s.h_slot, dense, hipHostMallocDefault), "hipHostMalloc targets") &&
                  e->check(hipHostMalloc((void**)&s.h_dense, dense, hipHostMallocDefault), "hipHostMalloc targets") &&
                  e->check(hipHostMalloc((void**)&s.h_rows, B * sizeof(int), hipHostMallocDefault), "hipHostMalloc loss rows") &&
                  e->check(hipHostMalloc((void**)&s.h_terms, B * kTerms * sizeof(float), hipHostMallocDefault), "hipHostMalloc terms") &&
                  e->check(hipHostMalloc((void**)&s.h_sums, kTerms * sizeof(double), hipHostMallocDefault), "hipHostMalloc sums") &&
                  e->check(hipMalloc((void**)&s.d_targets, dense), "hipMalloc targets") &&
                  e->check(hipMalloc((void**)&s.d_rows, B * sizeof(int)), "hipMalloc loss rows") &&
                  e->check(hipMalloc((void**)&s.d_terms, B * kTerms * sizeof(float)), "hipMalloc terms") &&
                  e->check(hipMalloc((void**)&s.d_sums, kTerms * sizeof(double)), "hipMalloc sums");
  if (!ok) {
    const std::string why = e->err;
    free_loss(e);
    (void)hipGetLastError();
    e->err = why;
    return false;
  }
  s.entry_of_slot.assign(B, -1);
  s.ready.store(true, std::memory_order_release);
  return true;
}

bool needs_aux(p3hip_engine* e, const char* who) {
  if (e->flags & P3HIP_FLAG_AUX) return true;
  e->err = std::string(who) + ": the engine was created without P3HIP_FLAG_AUX: nine of the loss terms read the aux record "
           "(pi_logits_aux, pi_logits_soft, the q heads, mcts_dist_logits), which only that flag computes";
  return false;
}

bool good_targets(p3hip_engine* e, const p3hip_targets& t, const char* who) {
  if (t.policy_aux >= 0 && t.policy_aux < P3HIP_NUM_MOVES) return true;
  e->err = std::string(who) + ": policy_aux is " + std::to_string(t.policy_aux) + ", a move index is 0 .. 361";
  return false;
}

// Uploads the n gathered entries (targets from src: h_dense, or h_slot when entry k is slot k; h_rows), computes their
// terms and brings back h_terms[0 .. n) and h_sums.
bool loss_entries(p3hip_engine* e, const float* src, int n) {
  auto& s = e->loss;
  p3::LossArgs a{e->d_out, e->d_aux, s.d_rows, s.d_targets, s.d_terms, s.d_sums, n};
  return e->check(hipMemcpyAsync(s.d_targets, src, (size_t)n * p3::kTgtStride * sizeof(float), hipMemcpyHostToDevice, e->stream), "H2D targets") &&
         e->check(hipMemcpyAsync(s.d_rows, s.h_rows, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream), "H2D loss rows") &&
         e->check(p3::launch_loss(a, e->stream), "launch k_loss_rows / k_loss_sum") &&
         e->check(hipMemcpyAsync(s.h_terms, s.d_terms, (size_t)n * kTerms * sizeof(float), hipMemcpyDeviceToHost, e->stream), "D2H terms") &&
         e->check(hipMemcpyAsync(s.h_sums, s.d_sums, kTerms * sizeof(double), hipMemcpyDeviceToHost, e->stream), "D2H sums") &&
         e->check(hipStreamSynchronize(e->stream), "sync");
}

}  // namespace

namespace eng {

void free_loss(p3hip_engine* e) {
  auto& s = e->loss;
  if (s.h_slot) hipHostFree(s.h_slot);
  if (s.h_dense) hipHostFree(s.h_dense);
  if (s.h_rows) hipHostFree(s.h_rows);
  if (s.h_terms) hipHostFree(s.h_terms);
  if (s.h_sums) hipHostFree(s.h_sums);
  hipFree(s.d_targets); hipFree(s.d_rows); hipFree(s.d_terms); hipFree(s.d_sums);
  s.h_slot = nullptr;
  s.h_dense = s.d_targets = nullptr;
  s.h_rows = s.d_rows = nullptr;
  s.h_terms = s.d_terms = nullptr;
  s.h_sums = s.d_sums = nullptr;
  s.ready.store(false, std::memory_order_release);
}

}  // namespace eng

extern "C" {

int p3hip_load_targets(p3hip_engine* e, int slot, const p3hip_targets* targets) {
  if (slot < 0 || slot >= e->batch || !targets) return 1;
  if (!good_targets(e, *targets, "p3hip_load_targets")) return 1;
  if (!ensure_loss(e)) return 1;
  p3::pack_targets(*targets, e->loss.h_slot + (size_t)slot * p3::kTgtStride);
  e->has_targets[slot] = 1;
  return 0;
}

int p3hip_loss(p3hip_engine* e, double sums[P3HIP_NUM_LOSS_TERMS], int* n_out) {
  auto& s = e->loss;
  for (int j = 0; j < kTerms; ++j) sums[j] = 0.0;
  if (n_out) *n_out = 0;
  if (!needs_aux(e, "p3hip_loss")) return 1;
  if (!s.ready.load(std::memory_order_acquire)) return 0;   // no targets were ever loaded
  if (!e->bind()) return 1;
  int n = 0;
  bool identity = true;   // entry k is slot k: the dense copy would be h_slot itself
  // no hook has overwritten d_out since the run, and the run went through the heads (P3HIP_DEBUG_STOP_BLOCK, p3hip_get_aux)
  const int stop = e->opt.stop_block;
  const bool rows_are_the_runs = e->run_seq == e->gather_seq && !(stop >= 0 && stop <= (int)e->plan.blocks.size());
  for (int slot = 0; slot < e->batch; ++slot) {
    const int row = rows_are_the_runs ? e->out_row_of(slot) : -1;
    s.entry_of_slot[slot] = -1;
    // (a slot loaded again since the run holds the next position's targets: not this row's)
    if (row < 0 || !e->has_targets[slot] || e->load_seq[slot] != e->run_load_seq[slot]) continue;
    if (slot != n) identity = false;
    s.h_rows[n] = row;
    s.entry_of_slot[slot] = n++;
  }
  if (!identity)
    for (int slot = 0; slot < e->batch; ++slot)
      if (s.entry_of_slot[slot] >= 0)
        memcpy(s.h_dense + (size_t)s.entry_of_slot[slot] * p3::kTgtStride, s.h_slot + (size_t)slot * p3::kTgtStride,
               p3::kTgtStride * sizeof(float));
  s.loss_run = e->run_seq;
  if (n == 0) return 0;
  if (!loss_entries(e, identity ? s.h_slot : s.h_dense, n)) { s.loss_run = -1; return 1; }
  memcpy(sums, s.h_sums, kTerms * sizeof(double));
  if (n_out) *n_out = n;
  return 0;
}

int p3hip_get_loss(p3hip_engine* e, int slot, float terms[P3HIP_NUM_LOSS_TERMS]) {
  if (slot < 0 || slot >= e->batch) return 1;
  const auto& s = e->loss;
  if (!s.ready.load(std::memory_order_acquire) || s.loss_run != e->run_seq || s.entry_of_slot[slot] < 0) return 2;
  memcpy(terms, s.h_terms + (size_t)s.entry_of_slot[slot] * kTerms, kTerms * sizeof(float));
  return 0;
}

int p3hip_debug_loss_rows(p3hip_engine* e, const float* raw, const float* aux, const p3hip_targets* targets, int n,
                          float* terms, double sums[P3HIP_NUM_LOSS_TERMS]) {
  if (!needs_aux(e, "p3hip_debug_loss_rows")) return 1;
  if (n < 1 || n > e->batch) { e->err = "p3hip_debug_loss_rows: n must be 1 .. batch size"; return 1; }
  for (int k = 0; k < n; ++k)
    if (!good_targets(e, targets[k], "p3hip_debug_loss_rows")) return 1;
  if (!ensure_loss(e) || !e->bind()) return 1;
  auto& s = e->loss;
  ++e->run_seq;   // rows 0 .. n - 1 of d_out and d_aux are no longer the last run's: scoring and losses stop answering
  auto put = [&](float* dst, int dst_stride, const float* src, int src_stride, int width, const char* what) {
    return e->check(hipMemcpy2DAsync(dst, (size_t)dst_stride * 4, src, (size_t)src_stride * 4, (size_t)width * 4, n,
                                     hipMemcpyHostToDevice, e->stream), what);
  };
  // p3hip_get_raw's layout, scattered back to where the heads write
  const struct { int src, dst, width; } seg[7] = {
      {0, p3::kOffMoveLogits, 362}, {362, p3::kOffOptLogits, 362}, {724, p3::kOffOutcomeLogits, 2},
      {726, p3::kOffScoreLogits, 800}, {1526, p3::kOffOwnership, 361}, {1887, p3::kOffErr2, 1}, {1888, p3::kOffGamma, 1}};
  for (const auto& g : seg)
    if (!put(e->d_out + g.dst, p3::kOutStride, raw + g.src, P3HIP_RAW_LEN, g.width, "H2D raw rows")) return 1;
  if (!put(e->d_aux, p3::kAuxStride, aux, P3HIP_AUX_LEN, P3HIP_AUX_LEN, "H2D aux records") ||
      // (the sources are pageable: drain the copies before anything else is staged)
      !e->check(hipStreamSynchronize(e->stream), "sync"))
    return 1;
  for (int k = 0; k < n; ++k) {
    p3::pack_targets(targets[k], s.h_dense + (size_t)k * p3::kTgtStride);
    s.h_rows[k] = k;
  }
  if (!loss_entries(e, s.h_dense, n)) return 1;
  memcpy(terms, s.h_terms, (size_t)n * kTerms * sizeof(float));
  memcpy(sums, s.h_sums, kTerms * sizeof(double));
  return 0;
}

}  // extern "C"
