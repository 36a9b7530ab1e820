// game_stats.h — the counters of a game runner, and their arithmetic.  A header of its own, so that measure_window.h
// (which sums them over the measured batches) needs nothing else of the host.
#pragma once

namespace p3 {

struct GameStats {
  long moves = 0, games = 0, evals = 0, black_wins = 0, cache_hits = 0;
  long bias_entries_pruned = 0;   // BiasCache::PruneUnused, self_play_thread.cc:730-733
  double bias_adj_abs_sum = 0;    // sum over moves of |obs_bias| of the root (self_play_thread.cc:639-641)

  // the one place that lists the fields again: a new counter goes into both
  GameStats& operator+=(const GameStats& o) {
    moves += o.moves; games += o.games; evals += o.evals; black_wins += o.black_wins; cache_hits += o.cache_hits;
    bias_entries_pruned += o.bias_entries_pruned;
    bias_adj_abs_sum += o.bias_adj_abs_sum;
    return *this;
  }
  GameStats operator-(const GameStats& o) const {
    GameStats d;
    d.moves = moves - o.moves; d.games = games - o.games; d.evals = evals - o.evals;
    d.black_wins = black_wins - o.black_wins; d.cache_hits = cache_hits - o.cache_hits;
    d.bias_entries_pruned = bias_entries_pruned - o.bias_entries_pruned;
    d.bias_adj_abs_sum = bias_adj_abs_sum - o.bias_adj_abs_sum;
    return d;
  }
};

}  // namespace p3
