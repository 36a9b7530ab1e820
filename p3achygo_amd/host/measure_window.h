// measure_window.h — the single definition of the benchmark's timed region.
//
// Every game group runs on its own: advance batches (until its games are past their openings), warm-up batches, then
// measured batches.  The measured region is ONE window for the whole job: it opens when the last group finishes its
// warm-up (at that run's completion) and closes
//   steps:    at the completion of the `limit`-th run after that, whichever groups those runs fall in,
//   seconds:  at the first completion `limit` seconds later,
//   rounds:   at the completion of the anchor lane's `limit`-th run after that (the anchor = the lane whose completion
//             opened the window), so both ends sit at the same phase of the groups' cycle on the GPU.
// Every run that completes inside the window is counted, with the game counters of the host phase that loaded it.  A
// lane leaves only when it sees the window closed, so the GPU stays under the same load for the whole window.
//
// No thread and no clock in here: the lanes' driver threads report their completions with the instants they took
// themselves (Completed), and the class owns the mutex that orders those reports.  tools/measure_window_check.cpp feeds it
// scripted sequences.
#pragma once
#include <chrono>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <vector>

#include "game_stats.h"

struct p3host_selfplay_stats {
  double seconds;            // wall time of the measured region
  long positions;            // network evaluations (engine slots loaded)
  long moves, games, black_wins;
  long batches;              // engine runs
  double gpu_seconds;        // time spent inside Evaluator::Run, summed over the groups
  double host_seconds;       // time spent advancing games (all groups, wall)
  long cache_hits;           // evaluations served by the per-game cache (not in `positions`)
  long advance_batches;      // untimed batches of the advance phase, all groups (p3host_selfplay_set_advance_limit)
  long games_past_opening;   // games past their raw-policy opening when the measured region began
  // batches x the least-squares slope of (batch index, completion instant) over the window: the same K steps, but
  // every completion weighs in instead of the first and the last (the groups' kernels interleave on the GPU, so
  // completions come in bursts and a short window's end points are +-1 batch); `seconds` is the window itself
  double seconds_fit;
  long rounds;               // p3host_selfplay_set_step_rounds: the anchor lane's batches inside the window (0 otherwise)
};

namespace p3 {

class MeasureWindow {
 public:
  using Instant = std::chrono::steady_clock::time_point;
  enum class Mode { kSeconds, kSteps, kRounds };
  // One engine run of a lane, as its driver thread saw it.
  struct Run {
    Instant start, done;      // around Evaluator::Run
    bool ok = true;
    // of the host phase that loaded the batch:
    GameStats delta;          // game counters it added
    double host_seconds = 0;
    long past_opening = 0;    // games of the group past their raw-policy opening
    bool in_opening = false;  // some game of the group is not
  };

  // advance_limit: untimed batches per group and lane, at most, to play every game past its opening (0 = none);
  // limit: seconds, batches or rounds, as `mode` says
  MeasureWindow(int groups, int lanes, long warmup_batches, int advance_limit, Mode mode, double limit)
      : warmup_batches_(warmup_batches), by_rounds_(mode == Mode::kRounds), by_steps_(mode == Mode::kSteps),
        seconds_(limit), count_limit_(mode == Mode::kSeconds ? 0 : (long)limit), groups_((size_t)groups) {
    // (a game in its opening has one evaluation in flight: every `lanes`-th batch)
    for (Group& g : groups_) g.adv_left = advance_limit * lanes;
  }

  // Lane `l` of group `h` finished a run.  True: the window is closed, the lane is to stop.
  bool Completed(int h, int l, const Run& run) {
    const Instant r0 = run.start, r1 = run.done;
    std::lock_guard<std::mutex> cl(mu_);
    Group& H = groups_[(size_t)h];
    if (!run.ok) failed_ = true;
    // a run belongs to the window by its completion instant, not by when its thread got the lock: r1 is taken
    // before the lock, so a run that completed before the window opened (or after it closed) can arrive here
    // with the phase already changed
    const bool inside = r1 > t0_ && (phase_ == 1 || (phase_ == 2 && by_rounds_ && r1 <= t1_));
    if (inside && phase_ != 0) {
      ++H.measured_batches;
      ++counted_;
      H.counted += run.delta;
      H.gpu_seconds += std::chrono::duration<double>(r1 - r0).count();
      H.host_seconds += run.host_seconds;
      if (phase_ == 1) {
        bool enough;
        if (by_rounds_) {
          // a round = one batch of every lane of every group; the anchor is ONE lane's completions
          const bool mine = h == anchor_ && l == anchor_lane_;
          if (mine) { ++anchor_rounds_; done_at_.push_back(std::chrono::duration<double>(r1 - t0_).count()); }
          enough = mine && anchor_rounds_ >= count_limit_;
        } else {
          done_at_.push_back(std::chrono::duration<double>(r1 - t0_).count());
          enough = by_steps_ ? counted_ >= count_limit_ : std::chrono::duration<double>(r1 - t0_).count() >= seconds_;
        }
        if (enough) { phase_ = 2; t1_ = r1; }
      }
    } else if (phase_ == 0 && !H.ready) {
      const bool in_opening = H.adv_left > 0 && run.in_opening;
      if (in_opening) { --H.adv_left; ++H.advance_batches; }
      else { H.adv_left = 0; ++H.warm; }
      if (H.warm >= warmup_batches_ || failed_) {
        H.ready = true;
        H.past_opening_at_start = run.past_opening;
        if (++groups_ready_ == (int)groups_.size()) { phase_ = failed_ ? 2 : 1; t0_ = t1_ = r1; anchor_ = h; anchor_lane_ = l; }
      }
    }
    if (phase_ == 1 && failed_) { phase_ = 2; t1_ = r1; }
    return phase_ == 2;
  }

  // Some run failed.  For the caller, after the lanes have stopped — as is Fill.
  bool failed() const { return failed_; }

  // Fills `out` from the window; returns the game counters summed over the measured batches.
  GameStats Fill(p3host_selfplay_stats* out) const {
    std::memset(out, 0, sizeof *out);
    GameStats total;
    for (const Group& H : groups_) {
      total += H.counted;
      out->batches += H.measured_batches;
      out->gpu_seconds += H.gpu_seconds;
      out->host_seconds += H.host_seconds;
      out->advance_batches += H.advance_batches;
      out->games_past_opening += H.past_opening_at_start;
    }
    out->positions = total.evals;
    out->moves = total.moves;
    out->games = total.games;
    out->black_wins = total.black_wins;
    out->cache_hits = total.cache_hits;
    out->seconds = std::chrono::duration<double>(t1_ - t0_).count();
    out->seconds_fit = out->seconds;
    out->rounds = anchor_rounds_;
    // completion k (1-based) at done_at[k - 1], the window's opening = completion 0 at 0
    // (by rounds: the anchor lane's completions, one per round)
    const size_t n = done_at_.size() + 1;
    if (n >= 4) {
      double sx = 0, sy = 0, sxx = 0, sxy = 0;
      for (size_t k = 0; k < n; ++k) {
        const double x = (double)k, y = k == 0 ? 0.0 : done_at_[k - 1];
        sx += x; sy += y; sxx += x * x; sxy += x * y;
      }
      const double slope = (n * sxy - sx * sy) / (n * sxx - sx * sx);
      if (slope > 0) out->seconds_fit = slope * (double)(n - 1);
    }
    return total;
  }

 private:
  struct Group {
    bool ready = false;
    long warm = 0;
    int adv_left = 0;
    long advance_batches = 0, past_opening_at_start = 0;
    long measured_batches = 0;
    GameStats counted;                           // game counters summed over the measured batches
    double gpu_seconds = 0, host_seconds = 0;    // inside Run / inside the host phases, measured region only
  };
  const long warmup_batches_;
  const bool by_rounds_, by_steps_;
  const double seconds_;
  const long count_limit_;
  std::mutex mu_;                      // guards everything below
  std::vector<Group> groups_;
  int phase_ = 0, groups_ready_ = 0;   // 0 advance + warm-up, 1 measuring, 2 over
  int anchor_ = -1, anchor_lane_ = 0;  // by rounds: the group (and lane) whose completions open and close the window
  long counted_ = 0, anchor_rounds_ = 0;
  bool failed_ = false;
  Instant t0_{}, t1_{};
  // completion instants, seconds since t0: of the counted batches, or (by rounds) of the anchor's
  std::vector<double> done_at_;
};

}  // namespace p3
