// scoring.cpp — the scoring entry points of the p3hip C ABI (include/p3hip.h, "scoring against labels on the device"):
// labels per slot in pinned memory, gathered by output row, scored by csrc/score.hip on the engine's stream.
#include <hip/hip_runtime.h>

#include <cstring>

#include "engine.h"
#include "score.h"

using namespace eng;

namespace {

constexpr int kTerms = P3HIP_NUM_SCORE_TERMS;
static_assert(sizeof(p3hip_labels) == 4 * (P3HIP_NUM_MOVES + 2), "p3hip_labels layout");

// The scoring buffers, made once.  p3hip_load_labels is called like p3hip_load_slot, from many threads at once.
bool ensure_scoring(p3hip_engine* e) {
  auto& s = e->scoring;
  if (s.ready.load(std::memory_order_acquire)) return true;
  std::lock_guard<std::mutex> lock(s.mu);
  if (s.ready.load(std::memory_order_relaxed)) return true;
  if (!e->bind()) return false;
  const size_t B = (size_t)e->batch;
  const bool ok = e->check(hipHostMalloc((void**)&s.h_slot, B * sizeof(p3hip_labels), hipHostMallocDefault), "hipHostMalloc labels") &&
                  e->check(hipHostMalloc((void**)&s.h_dense, B * sizeof(p3hip_labels), hipHostMallocDefault), "hipHostMalloc labels") &&
                  e->check(hipHostMalloc((void**)&s.h_rows, B * sizeof(int), hipHostMallocDefault), "hipHostMalloc score rows") &&
                  e->check(hipHostMalloc((void**)&s.h_terms, B * kTerms * sizeof(float), hipHostMallocDefault), "hipHostMalloc terms") &&
                  e->check(hipHostMalloc((void**)&s.h_sums, kTerms * sizeof(double), hipHostMallocDefault), "hipHostMalloc sums") &&
                  e->check(hipMalloc((void**)&s.d_labels, B * sizeof(p3hip_labels)), "hipMalloc labels") &&
                  e->check(hipMalloc((void**)&s.d_rows, B * sizeof(int)), "hipMalloc score rows") &&
                  e->check(hipMalloc((void**)&s.d_terms, B * kTerms * sizeof(float)), "hipMalloc terms") &&
                  e->check(hipMalloc((void**)&s.d_sums, kTerms * sizeof(double)), "hipMalloc sums");
  if (!ok) {
    const std::string why = e->err;
    free_scoring(e);
    (void)hipGetLastError();
    e->err = why;
    return false;
  }
  s.entry_of_slot.assign(B, -1);
  s.ready.store(true, std::memory_order_release);
  return true;
}

// Uploads the n gathered entries (h_dense, h_rows), scores them and brings back h_terms[0 .. n) and h_sums.
bool score_entries(p3hip_engine* e, int n) {
  auto& s = e->scoring;
  p3::ScoreArgs a{e->d_out, s.d_rows, s.d_labels, s.d_terms, s.d_sums, n};
  return e->check(hipMemcpyAsync(s.d_labels, s.h_dense, (size_t)n * sizeof(p3hip_labels), hipMemcpyHostToDevice, e->stream), "H2D labels") &&
         e->check(hipMemcpyAsync(s.d_rows, s.h_rows, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream), "H2D score rows") &&
         e->check(p3::launch_score(a, e->stream), "launch k_score_rows / k_score_sum") &&
         e->check(hipMemcpyAsync(s.h_terms, s.d_terms, (size_t)n * kTerms * sizeof(float), hipMemcpyDeviceToHost, e->stream), "D2H terms") &&
         e->check(hipMemcpyAsync(s.h_sums, s.d_sums, kTerms * sizeof(double), hipMemcpyDeviceToHost, e->stream), "D2H sums") &&
         e->check(hipStreamSynchronize(e->stream), "sync");
}

}  // namespace

namespace eng {

void free_scoring(p3hip_engine* e) {
  auto& s = e->scoring;
  if (s.h_slot) hipHostFree(s.h_slot);
  if (s.h_dense) hipHostFree(s.h_dense);
  if (s.h_rows) hipHostFree(s.h_rows);
  if (s.h_terms) hipHostFree(s.h_terms);
  if (s.h_sums) hipHostFree(s.h_sums);
  hipFree(s.d_labels); hipFree(s.d_rows); hipFree(s.d_terms); hipFree(s.d_sums);
  s.h_slot = s.h_dense = s.d_labels = nullptr;
  s.h_rows = s.d_rows = nullptr;
  s.h_terms = s.d_terms = nullptr;
  s.h_sums = s.d_sums = nullptr;
  s.ready.store(false, std::memory_order_release);
}

}  // namespace eng

extern "C" {

int p3hip_load_labels(p3hip_engine* e, int slot, const p3hip_labels* labels) {
  if (slot < 0 || slot >= e->batch || !labels) return 1;
  if (!ensure_scoring(e)) return 1;
  memcpy(e->scoring.h_slot + slot, labels, sizeof(p3hip_labels));
  e->has_labels[slot] = 1;
  return 0;
}

int p3hip_score(p3hip_engine* e, double sums[P3HIP_NUM_SCORE_TERMS], int* n_scored) {
  auto& s = e->scoring;
  for (int j = 0; j < kTerms; ++j) sums[j] = 0.0;
  if (n_scored) *n_scored = 0;
  if (!s.ready.load(std::memory_order_acquire)) return 0;   // no labels were ever loaded
  if (!e->bind()) return 1;
  int n = 0;
  const bool rows_are_the_runs = e->run_seq == e->gather_seq;   // no hook has overwritten d_out since the run
  for (int slot = 0; slot < e->batch; ++slot) {
    const int row = rows_are_the_runs ? e->out_row_of(slot) : -1;
    s.entry_of_slot[slot] = -1;
    // (a slot loaded again since the run holds the next position's labels: not this row's)
    if (row < 0 || !e->has_labels[slot] || e->load_seq[slot] != e->run_load_seq[slot]) continue;
    memcpy(s.h_dense + n, s.h_slot + slot, sizeof(p3hip_labels));
    s.h_rows[n] = row;
    s.entry_of_slot[slot] = n++;
  }
  s.scored_run = e->run_seq;
  if (n == 0) return 0;
  if (!score_entries(e, n)) { s.scored_run = -1; return 1; }
  memcpy(sums, s.h_sums, kTerms * sizeof(double));
  if (n_scored) *n_scored = n;
  return 0;
}

int p3hip_get_score(p3hip_engine* e, int slot, float terms[P3HIP_NUM_SCORE_TERMS]) {
  if (slot < 0 || slot >= e->batch) return 1;
  const auto& s = e->scoring;
  if (!s.ready.load(std::memory_order_acquire) || s.scored_run != e->run_seq || s.entry_of_slot[slot] < 0) return 2;
  memcpy(terms, s.h_terms + (size_t)s.entry_of_slot[slot] * kTerms, kTerms * sizeof(float));
  return 0;
}

int p3hip_debug_score_rows(p3hip_engine* e, const float* move_probs, const float* value_probs, const float* score_probs,
                           const p3hip_labels* labels, int n, float* terms, double sums[P3HIP_NUM_SCORE_TERMS]) {
  if (n < 1 || n > e->batch) { e->err = "p3hip_debug_score_rows: n must be 1 .. batch size"; return 1; }
  if (!ensure_scoring(e) || !e->bind()) return 1;
  auto& s = e->scoring;
  ++e->run_seq;   // rows 0 .. n - 1 of d_out are no longer the last run's: p3hip_score / p3hip_get_score stop answering
  const size_t pitch = p3::kOutStride * sizeof(float);
  auto put = [&](const float* src, int off, int width, const char* what) {
    return e->check(hipMemcpy2DAsync(e->d_out + off, pitch, src, (size_t)width * 4, (size_t)width * 4, n, hipMemcpyHostToDevice, e->stream), what);
  };
  if (!put(move_probs, p3::kOffMoveProbs, P3HIP_NUM_MOVES, "H2D move probs") ||
      !put(value_probs, p3::kOffValueProbs, P3HIP_NUM_VALUE_LOGITS, "H2D value probs") ||
      !put(score_probs, p3::kOffScoreProbs, P3HIP_NUM_SCORE_LOGITS, "H2D score probs") ||
      // (the sources are pageable: drain the copies before anything else is staged)
      !e->check(hipStreamSynchronize(e->stream), "sync"))
    return 1;
  memcpy(s.h_dense, labels, (size_t)n * sizeof(p3hip_labels));
  for (int k = 0; k < n; ++k) s.h_rows[k] = k;
  if (!score_entries(e, n)) return 1;
  memcpy(terms, s.h_terms, (size_t)n * kTerms * sizeof(float));
  memcpy(sums, s.h_sums, kTerms * sizeof(double));
  return 0;
}

}  // extern "C"
