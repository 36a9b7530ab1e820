// measure_window_check.cpp — the benchmark's timed region (p3achygo_amd/host/measure_window.h) on scripted completion
// sequences with hand-made instants: no thread, no pool, no evaluator.  Every expectation below is worked out by hand from
// the window's rules and written beside the sequence.  Built with the address and undefined-behaviour sanitizers and run as
// a program of its own by tests/test_measure_window_cpu.py.
//
// The rules, for reference while reading the sequences:
//   * a group spends at most advance_limit x lanes untimed ADVANCE batches while its lanes report "in opening", then
//     `warmup` WARM-UP batches; then it is ready, and its further completions before the opening are ignored;
//   * the window opens at the completion that makes the last group ready (t0), and that lane is the anchor;
//   * a completion is inside when its instant is > t0 and the window is open — or, by rounds only, closed with the
//     instant <= t1 (a report that arrives late);
//   * steps: closes at the limit-th counted completion; seconds: at the first counted completion >= limit after t0;
//     rounds: at the anchor LANE's limit-th counted completion;
//   * a failed run makes its group (and every group that reports after it) ready at once, and closes an open window at
//     that completion.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../p3achygo_amd/host/measure_window.h"

using p3::GameStats;
using p3::MeasureWindow;
using Mode = MeasureWindow::Mode;

static int g_checks = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checks;                                                                  \
    if (!(cond)) {                                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

static MeasureWindow::Instant At(long us) { return MeasureWindow::Instant{} + std::chrono::microseconds(us); }
static double Sec(long us) { return std::chrono::duration<double>(std::chrono::microseconds(us)).count(); }

// a run that took `gpu_us` on the engine and completed at `done_us`; its host phase added `evals` evaluations (and
// 2 x evals moves, so that a sum that mixes the fields up shows)
static MeasureWindow::Run R(long done_us, long evals, long gpu_us = 4, bool ok = true) {
  MeasureWindow::Run r;
  r.start = At(done_us - gpu_us);
  r.done = At(done_us);
  r.ok = ok;
  r.delta.evals = evals;
  r.delta.moves = 2 * evals;
  r.host_seconds = 0.5;
  return r;
}
static MeasureWindow::Run Opening(long done_us, bool in_opening, long past_opening) {
  MeasureWindow::Run r = R(done_us, 1);
  r.in_opening = in_opening;
  r.past_opening = past_opening;
  return r;
}

// Steps: three groups, warm-up 1, limit 5.
static void Steps() {
  MeasureWindow w(3, 1, 1, 0, Mode::kSteps, 5);
  p3host_selfplay_stats s;
  CHECK(!w.Completed(0, 0, R(10, 1)));      // group 0 ready
  CHECK(!w.Completed(1, 0, R(20, 1)));      // group 1 ready
  CHECK(!w.Completed(0, 0, R(30, 1)));      // group 0 again, before the opening: ignored
  CHECK(!w.Completed(2, 0, R(40, 1)));      // the last group's warm-up completion: the window opens, t0 = 40
  CHECK(!w.Completed(0, 0, R(50, 100)));    // 1
  CHECK(!w.Completed(0, 0, R(60, 200)));    // 2: whichever groups they fall in
  CHECK(!w.Completed(1, 0, R(70, 400)));    // 3
  CHECK(!w.Completed(2, 0, R(80, 800)));    // 4
  CHECK(w.Completed(0, 0, R(90, 1600)));    // 5: closed, t1 = 90
  CHECK(w.Completed(1, 0, R(85, 3200)));    // completed inside, reported after the close: by steps NOT counted
  CHECK(w.Completed(2, 0, R(95, 6400)));    // after the close
  w.Fill(&s);
  CHECK(s.batches == 5 && s.positions == 100 + 200 + 400 + 800 + 1600 && s.moves == 2 * s.positions);
  CHECK(s.seconds == Sec(50) && s.rounds == 0 && s.advance_batches == 0);
  CHECK(std::fabs(s.gpu_seconds - 5 * Sec(4)) < 1e-15 && s.host_seconds == 2.5);   // of the counted five only
  CHECK(!w.failed());
}

// Rounds: two groups of two lanes, warm-up 1, limit 2.  Only the anchor lane's completions advance `rounds`.
static void Rounds() {
  MeasureWindow w(2, 2, 1, 0, Mode::kRounds, 2);
  p3host_selfplay_stats s;
  CHECK(!w.Completed(0, 0, R(10, 1)));      // group 0 ready (a group's warm-up counts its lanes' batches together)
  CHECK(!w.Completed(0, 1, R(15, 1)));      // ignored
  CHECK(!w.Completed(1, 0, R(20, 1)));      // opens: t0 = 20, anchor = group 1, lane 0
  CHECK(!w.Completed(0, 1, R(20, 7)));      // instant == t0, reported after the opening: not counted
  CHECK(!w.Completed(0, 0, R(18, 7)));      // instant < t0, reported after the opening: not counted
  CHECK(!w.Completed(0, 0, R(30, 100)));    // counted, rounds 0
  CHECK(!w.Completed(1, 1, R(35, 100)));    // the anchor's group, the other lane: counted, rounds 0
  CHECK(!w.Completed(1, 0, R(40, 100)));    // the anchor: rounds 1
  CHECK(!w.Completed(0, 1, R(45, 100)));    // counted
  CHECK(w.Completed(1, 0, R(60, 100)));     // the anchor: rounds 2, closed, t1 = 60
  CHECK(w.Completed(0, 0, R(55, 100)));     // instant <= t1, reported after the close: counted
  CHECK(w.Completed(0, 1, R(60, 100)));     // instant == t1: counted
  CHECK(w.Completed(1, 1, R(61, 7)));       // instant > t1: not counted
  CHECK(w.Completed(1, 0, R(59, 100)));     // the anchor itself, late: counted as a batch, but the rounds stay
  w.Fill(&s);
  CHECK(s.batches == 8 && s.positions == 800 && s.rounds == 2 && s.seconds == Sec(40));
  CHECK(s.seconds_fit == s.seconds);        // two completions of the anchor: fewer than three, no fit
}

// The advance phase: two lanes, advance limit 3 (so 6 batches per group at most), warm-up 2, one measured step.
static void Advance() {
  MeasureWindow w(3, 2, 2, 3, Mode::kSteps, 1);
  p3host_selfplay_stats s;
  // group 1 is past its opening at once: straight to warm-up, ready after two batches
  CHECK(!w.Completed(1, 0, Opening(1, false, 40)));
  CHECK(!w.Completed(1, 1, Opening(2, false, 41)));     // ready: 41 games past the opening at its start
  // group 2 leaves its opening after two batches; a later "in opening" report does not bring the advance phase back
  CHECK(!w.Completed(2, 0, Opening(3, true, 10)));
  CHECK(!w.Completed(2, 1, Opening(4, true, 20)));
  CHECK(!w.Completed(2, 0, Opening(5, false, 30)));     // warm-up 1
  CHECK(!w.Completed(2, 1, Opening(6, true, 29)));      // warm-up 2: ready, 29
  // group 0 never leaves its opening: 3 x 2 advance batches, then it warms up all the same
  for (int i = 0; i < 6; ++i) CHECK(!w.Completed(0, i % 2, Opening(10 + i, true, 5)));
  CHECK(!w.Completed(0, 0, Opening(20, true, 6)));      // warm-up 1
  CHECK(!w.Completed(0, 1, Opening(21, true, 7)));      // warm-up 2: ready, 7; the window opens
  CHECK(w.Completed(1, 0, Opening(30, false, 48)));     // the one measured step
  w.Fill(&s);
  CHECK(s.advance_batches == 0 + 2 + 6 && s.games_past_opening == 41 + 29 + 7 && s.batches == 1 && s.seconds == Sec(9));
}

// A failed run during warm-up ends the job with an empty window; one inside the window closes it at that completion.
static void Failures() {
  p3host_selfplay_stats s;
  {
    MeasureWindow w(2, 1, 3, 0, Mode::kSteps, 5);
    CHECK(!w.Completed(0, 0, R(10, 1)));                 // warm-up 1 of 3
    CHECK(!w.Completed(1, 0, R(20, 1, 4, false)));       // fails: group 1 ready at once; group 0 is not yet
    CHECK(w.Completed(0, 0, R(30, 1)));                  // group 0 ready for the same reason: opens closed, t0 = t1 = 30
    CHECK(w.Completed(1, 0, R(40, 1)));
    w.Fill(&s);
    CHECK(w.failed() && s.batches == 0 && s.positions == 0 && s.seconds == 0 && s.seconds_fit == 0);
  }
  {
    MeasureWindow w(2, 1, 1, 0, Mode::kSteps, 10);
    CHECK(!w.Completed(0, 0, R(10, 1)));
    CHECK(!w.Completed(1, 0, R(20, 1)));                 // opens, t0 = 20
    CHECK(!w.Completed(0, 0, R(30, 100)));
    CHECK(w.Completed(1, 0, R(40, 100, 4, false)));      // fails inside: counted like any completion, and closes: t1 = 40
    CHECK(w.Completed(0, 0, R(50, 100)));
    w.Fill(&s);
    CHECK(w.failed() && s.batches == 2 && s.seconds == Sec(20));
  }
  {
    MeasureWindow w(2, 1, 1, 0, Mode::kRounds, 10);      // the same by rounds, the failure not on the anchor
    CHECK(!w.Completed(0, 0, R(10, 1)));
    CHECK(!w.Completed(1, 0, R(20, 1)));                 // opens, anchor = group 1
    CHECK(w.Completed(0, 0, R(30, 100, 4, false)));      // closes at 30
    w.Fill(&s);
    CHECK(w.failed() && s.batches == 1 && s.rounds == 0 && s.seconds == Sec(10));
  }
}

// one group, warm-up 1 at 1 s, then completions at the given quarter seconds after the opening; steps = their number
static p3host_selfplay_stats Fit(std::initializer_list<long> quarters) {
  MeasureWindow w(1, 1, 1, 0, Mode::kSteps, (double)quarters.size());
  p3host_selfplay_stats s;
  w.Completed(0, 0, R(1000000, 1));
  size_t k = 0;
  for (long q : quarters) CHECK(w.Completed(0, 0, R(1000000 + 250000 * q, 1)) == (++k == quarters.size()));
  w.Fill(&s);
  return s;
}
static void Fits() {
  // completions at exact multiples of d = 0.25 s (every instant, sum and product below is exact in binary):
  // the slope is d, seconds_fit = n d
  p3host_selfplay_stats s = Fit({1, 2, 3, 4});
  CHECK(s.seconds == 1.0 && s.seconds_fit == 4 * 0.25);
  s = Fit({1, 2, 3, 4, 5, 6, 7});
  CHECK(s.seconds == 1.75 && s.seconds_fit == 7 * 0.25);
  // a burst and a gap: x = 0..4, y = 0, .25, .5, .75, 2: sx = 10, sy = 3.5, sxx = 30, sxy = 11.5,
  // slope = (5 x 11.5 - 10 x 3.5) / (5 x 30 - 100) = 0.45, seconds_fit = 4 x 0.45 = 1.8 — not the window's 2.0
  s = Fit({1, 2, 3, 8});
  CHECK(s.seconds == 2.0 && std::fabs(s.seconds_fit - 1.8) < 1e-12);
  // three completions are enough (n = 4 points with the opening): y = 0, .25, .5, 1: sx = 6, sy = 1.75, sxx = 14,
  // sxy = 4.25, slope = (4 x 4.25 - 6 x 1.75) / (4 x 14 - 36) = 0.325, seconds_fit = 0.975
  s = Fit({1, 2, 4});
  CHECK(s.seconds == 1.0 && std::fabs(s.seconds_fit - 0.975) < 1e-12);
  // fewer than three completions: seconds_fit = seconds
  s = Fit({1, 4});
  CHECK(s.seconds == 1.0 && s.seconds_fit == 1.0);
  s = Fit({3});
  CHECK(s.seconds == 0.75 && s.seconds_fit == 0.75);
}

// Seconds: closes at the first completion at or past `seconds` after the opening.
static void Seconds() {
  p3host_selfplay_stats s;
  {
    MeasureWindow w(1, 1, 1, 0, Mode::kSeconds, 1.0);
    CHECK(!w.Completed(0, 0, R(1000000, 1)));     // opens at 1 s
    CHECK(!w.Completed(0, 0, R(1500000, 10)));    // 0.5 s
    CHECK(w.Completed(0, 0, R(2000000, 10)));     // exactly 1.0 s: at, so closed
    w.Fill(&s);
    CHECK(s.batches == 2 && s.seconds == 1.0);
  }
  {
    MeasureWindow w(1, 1, 1, 0, Mode::kSeconds, 1.0);
    CHECK(!w.Completed(0, 0, R(1000000, 1)));
    CHECK(!w.Completed(0, 0, R(1999999, 10)));    // just short
    CHECK(w.Completed(0, 0, R(2250000, 10)));     // past: the window is as long as this completion makes it
    w.Fill(&s);
    CHECK(s.batches == 2 && s.seconds == 1.25);
  }
}

// The counters of the counted batches come back whole (GameStats' own arithmetic, every field).
static void Counters() {
  MeasureWindow w(1, 1, 1, 0, Mode::kSteps, 2);
  w.Completed(0, 0, R(10, 1));
  MeasureWindow::Run r = R(20, 0);
  r.delta.moves = 1; r.delta.games = 2; r.delta.evals = 3; r.delta.black_wins = 4; r.delta.cache_hits = 5;
  r.delta.bias_entries_pruned = 6; r.delta.bias_adj_abs_sum = 0.5;
  w.Completed(0, 0, r);
  r.done = At(30);
  w.Completed(0, 0, r);
  p3host_selfplay_stats s;
  const GameStats t = w.Fill(&s);
  CHECK(s.moves == 2 && s.games == 4 && s.positions == 6 && s.black_wins == 8 && s.cache_hits == 10);
  CHECK(t.bias_entries_pruned == 12 && t.bias_adj_abs_sum == 1.0 && t.evals == 6);
  const GameStats d = t - r.delta;
  CHECK(d.moves == 1 && d.games == 2 && d.evals == 3 && d.black_wins == 4 && d.cache_hits == 5 &&
        d.bias_entries_pruned == 6 && d.bias_adj_abs_sum == 0.5);
}

int main() {
  Steps();
  Rounds();
  Advance();
  Failures();
  Fits();
  Seconds();
  Counters();
  std::printf("%d checks\nok\n", g_checks);
  return 0;
}
