// selfplay_tsan_main.cpp — the self-play scheduler under ThreadSanitizer, as a program of its own: linked with the host
// sources compiled -fsanitize=thread (`make tsan_check` in p3achygo_amd/host), nothing is loaded into an interpreter.
// One run over the hash evaluator with two groups of two lanes, four playouts in flight and slow games, so that lanes,
// the spare-row pass and the straggler hand-over all happen.  Exits non-zero on a ThreadSanitizer report (the runtime's
// own exit code), on a failed run, or when no host phase handed a straggler over.
#include <cstdint>
#include <cstdio>

#include "../p3achygo_amd/host/measure_window.h"   // p3host_selfplay_stats

extern "C" {
void p3host_selfplay_set_groups(int n);
void p3host_selfplay_set_lanes(int lanes, int max_inflight);
void p3host_selfplay_set_test_slow_games(long us);
void p3host_selfplay_set_step_rounds(long rounds);
void p3host_selfplay_last_handed_over(long* phases, long* games);
int p3host_selfplay_run(const char* engine_lib, const char* weights, int device, int num_games, int num_threads, int default_n,
                        int default_k, int selected_n, int selected_k, int max_moves, double seconds, int warmup_batches,
                        uint64_t seed, p3host_selfplay_stats* out, char* err);
}

int main() {
  p3host_selfplay_set_groups(2);
  p3host_selfplay_set_lanes(2, 4);
  p3host_selfplay_set_test_slow_games(3000);
  p3host_selfplay_set_step_rounds(12);
  p3host_selfplay_stats st;
  char err[256] = "";
  const int rc = p3host_selfplay_run("hash", nullptr, 0, /*num_games=*/128, /*num_threads=*/4, /*default_n=*/16, /*default_k=*/4,
                                     /*selected_n=*/16, /*selected_k=*/4, /*max_moves=*/600, /*seconds=*/60.0,
                                     /*warmup_batches=*/2, /*seed=*/7, &st, err);
  long phases = 0, games = 0;
  p3host_selfplay_last_handed_over(&phases, &games);
  std::printf("rc %d%s%s: %ld batches, %ld rounds, %ld positions, %ld moves, %.3f s; handed over: %ld phases, %ld games\n", rc,
              err[0] ? " " : "", err, st.batches, st.rounds, st.positions, st.moves, st.seconds, phases, games);
  if (rc != 0) return 1;
  if (st.rounds != 12) { std::printf("FAILED: the window did not run its 12 rounds\n"); return 1; }
  if (phases <= 0 || games <= 0) { std::printf("FAILED: no host phase handed a straggler over\n"); return 1; }
  std::printf("ok\n");
  return 0;
}
