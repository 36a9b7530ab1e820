// selfplay.cc — the self-play driver: thousands of concurrent games, their search leaves
// coalesced into large inference batches for the engine behind include/p3hip.h.
//
// The game itself is game_runner.h.  Scheduling is new (the reference runs one OS thread per game and a 400 us batching
// timeout, nn_interface.cc:279-404): games are resumable state machines (search.h) split in
// N groups, each group bound to its own engine instance; while the GPU evaluates the leaves
// of one group, a pool of host threads (worker_pool.h) consumes the results of the others, advances those
// games to their next leaf and loads the next batch — so every batch holds one leaf of
// (nearly) every game of its group and the GPU never waits for a timeout.  What a run measures is decided in
// measure_window.h.  The reference's blocking thread-per-game NNInterface is kept too (nn_interface.h) for callers
// written against it; the evaluation matches are eval_match.cc.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>

#include "game_runner.h"
#include "measure_window.h"
#include "worker_pool.h"

namespace p3 {

// ---- scheduler -----------------------------------------------------------------------------
// One game group: its games and its LANES.  A lane is an engine instance with its own stream and a driver
// thread that alternates "evaluate the lane's batch" (Evaluator::Run: H2D, forward pass, D2H) and the lane's host
// phase "hand its results to the games, advance every game to its next leaf, load the leaves" (ParallelFors on the
// shared pool).  With one lane (the default) host and GPU alternate within the group and it is the other groups
// that keep the GPU busy.  With two, the host phases of the lanes alternate — while one lane's batch is on the GPU
// the other lane's results are consumed and its next batch is filled — which needs games that can have leaves in
// both batches at once: GameRunner::TryAdvance with several playouts in flight.
struct Lane {
  std::unique_ptr<Evaluator> eval;
  std::thread driver;
  std::atomic<int> count{0};   // slots loaded for the next run
};
struct Group {
  std::vector<std::unique_ptr<Lane>> lanes;
  std::vector<std::unique_ptr<GameRunner>> games;
  std::vector<p3hip_features> feats;
  // whose host phase is next (the lanes' host phases alternate strictly, so a game's results arrive in request order)
  std::mutex turn_mu;
  std::condition_variable turn_cv;
  int turn = 0;
  bool quit = false;
  GameStats prev;              // game counters at the end of the last host phase (host phases only)
  // Stragglers (two or more lanes): a host phase that is waiting for a last few slow games while the GPU has run dry hands
  // them over — its batch leaves without them, they finish on the pool (`late`), and the group's next host phase starts by
  // waiting for them and loads what they asked for into ITS batch.  `settled[g]` = game g's task of the current phase has
  // ended (its counters may be read); `snap` = every game's counters as last read settled.
  WorkerPool::JobRef late;
  std::unique_ptr<std::atomic<uint8_t>[]> settled;
  std::vector<GameStats> snap;
  std::vector<uint8_t> snap_past_opening;
  std::atomic<int> waiting{0};   // lane drivers waiting for their turn (their runs are done: the GPU is about to idle)
  long handed_over_phases = 0, handed_over_games = 0, phase_no = 0;

  GameStats Totals() const {
    GameStats t;
    for (const GameStats& g : snap) t += g;
    return t;
  }
};

// What the p3host_selfplay_set_* entry points set, for the runs after them.
struct SelfPlayOptions {
  std::string rec_dir, rec_worker = "0";
  int rec_gen = 0, rec_flush_interval = 128;   // --flush_interval, selfplay/main.cc:35
  bool init_state_sampling = true;
  float use_seen_state_prob = 0.5f, sel_mult_base = 0.0f, sel_mult_scale = 1.0f;
  float bias_cache_lambda = 0.0f, bias_cache_alpha = 0.8f;
  bool early_stopping = false;
  bool device_symmetry = false;
  bool graph_any = false;
  std::string calibration_file;
  int num_groups = 2;
  int num_lanes = 1, max_inflight = 1;
  long step_limit = 0;    // > 0: the measured region ends after this many engine batches
  long step_rounds = 0;   // > 0: the measured region is this many ROUNDS (one batch of every group), anchored on one lane
  int advance_limit = 0;  // > 0: untimed batches per group, at most, to play every game past its raw-policy opening
  long test_slow_us = 0;  // tests: some games sleep this long in some host phases (a stand-in for a slow ladder read-out)
};
// What the p3host_selfplay_last_* entry points read: of the last run (the bias-cache figures: or single game).
struct SelfPlayLastRun {
  long bias_pruned = 0;
  double bias_adj = 0;
  long handed_over_phases = 0, handed_over_games = 0;
  std::vector<uint64_t> first_game_digests;   // one per game runner
  long reuse_added = 0, examples = 0;
};

// One p3host_selfplay_run: Build, Run, Collect.
class SelfPlayJob {
 public:
  SelfPlayJob(const SelfPlayOptions& opt, int num_threads, int warmup_batches, double seconds)
      : opt_(opt), NG(opt.num_groups), NL(opt.num_lanes), depth_(NL > 1 ? opt.max_inflight : 1),
        groups_((size_t)NG), pool_(num_threads > 0 ? num_threads : 1),
        // rounds win over steps, steps over seconds
        window_(NG, NL, warmup_batches, opt.advance_limit,
                opt.step_rounds > 0 ? MeasureWindow::Mode::kRounds
                                    : opt.step_limit > 0 ? MeasureWindow::Mode::kSteps : MeasureWindow::Mode::kSeconds,
                opt.step_rounds > 0 ? (double)opt.step_rounds : opt.step_limit > 0 ? (double)opt.step_limit : seconds),
        phase_stats_(getenv("P3HOST_PHASE_STATS") != nullptr) {
    for (auto& c : phase_hist_) c.store(0);
  }

  // The evaluators and the games: `cfg` holds the caller's search sizes, the rest of it comes from the options.  False
  // with a message in `err` (256 bytes).
  bool Build(const char* engine_lib, const char* weights, int device, int num_games, SelfPlayConfig cfg, uint64_t seed,
             char* err) {
    cfg.init_state_sampling = opt_.init_state_sampling;
    cfg.use_seen_state_prob = opt_.use_seen_state_prob;
    cfg.sel_mult_base = opt_.sel_mult_base;
    cfg.sel_mult_scale_factor = opt_.sel_mult_scale;
    cfg.bias_cache_lambda = opt_.bias_cache_lambda;
    cfg.bias_cache_alpha = opt_.bias_cache_alpha;
    cfg.early_stopping_enabled = opt_.early_stopping;
    dev_sym_ = opt_.device_symmetry && engine_lib && engine_lib[0] && std::strcmp(engine_lib, "hash") != 0;
    cfg.device_symmetry = dev_sym_;
    cfg.calibration = ParseCalibrationFile(opt_.calibration_file);
    cfg.fork_params = ForkParams::ForReuse(opt_.use_seen_state_prob);
    reuse_ = std::make_unique<ReuseBuffer>(seed ^ 0x676f6578706c6f69ull);
    cfg.reuse = reuse_.get();
    if (!opt_.rec_dir.empty()) {
      ::mkdir((opt_.rec_dir + "/sgf").c_str(), 0755);
      ::mkdir((opt_.rec_dir + "/chunks").c_str(), 0755);
      recorder_.reset(new GameRecorder(opt_.rec_dir, opt_.rec_gen, opt_.rec_worker, opt_.rec_flush_interval));
      cfg.recorder = recorder_.get();
    }
    if (num_games < NG) num_games = NG;
    for (int h = 0; h < NG; ++h) {
      Group& H = groups_[h];
      const int ng = num_games / NG + (h < num_games % NG ? 1 : 0);
      for (int l = 0; l < NL; ++l) {
        H.lanes.emplace_back(new Lane());
        // one engine per lane, all on this GPU (device symmetry: one copy per slot, so as many rows as slots)
        H.lanes[l]->eval = MakeEvaluator(engine_lib, ng, err, [&](HipEvaluator& e) {
          return e.Open(engine_lib, weights, ng, device, P3HIP_FLAG_SHARED_DEVICE | (dev_sym_ ? P3HIP_FLAG_SYMMETRY_SLOT : 0u) |
                        (opt_.graph_any ? P3HIP_FLAG_LAUNCH_GRAPH_ANY : 0u), dev_sym_ ? ng : 0);
        });
        if (!H.lanes[l]->eval) return false;
      }
      for (int g = 0; g < ng; ++g) {
        // documented per-game seed (replaces absl::HashOf(worker_id, thread_id), main.cc:244)
        uint64_t s = seed * 0x9E3779B97F4A7C15ull + (uint64_t)(h * 1000003 + g) * 0xBF58476D1CE4E5B9ull;
        H.games.emplace_back(new GameRunner(cfg, s));
      }
      H.feats.resize((size_t)ng);
      H.settled.reset(new std::atomic<uint8_t>[(size_t)ng]);
      H.snap.resize((size_t)ng);
      H.snap_past_opening.assign((size_t)ng, 0);
      for (int g = 0; g < ng; ++g) {
        H.settled[g].store(1);
        H.snap[g] = H.games[g]->stats();
      }
      H.prev = H.Totals();
    }
    return true;
  }

  // One driver thread per lane, until the window has closed.
  void Run() {
    for (int h = 0; h < NG; ++h)
      for (int l = 0; l < NL; ++l) groups_[h].lanes[l]->driver = std::thread([this, h, l] { LaneLoop(h, l); });
    for (auto& H : groups_)
      for (auto& L : H.lanes) L->driver.join();
  }

  // The results of a finished Run: `last`, `out` (may be null), and the return code of p3host_selfplay_run.
  int Collect(SelfPlayLastRun* last, p3host_selfplay_stats* out, char* err) {
    last->handed_over_phases = last->handed_over_games = 0;
    for (auto& H : groups_) {
      if (H.late) { pool_.Wait(H.late); H.late.reset(); }   // before the games go away
      last->handed_over_phases += H.handed_over_phases;
      last->handed_over_games += H.handed_over_games;
    }
    if (phase_stats_) {
      std::fprintf(stderr, "host phases by duration (ms, last bin >= 15):");
      for (int b = 0; b < 16; ++b) std::fprintf(stderr, " %ld", phase_hist_[b].load());
      std::fprintf(stderr, "\n");
    }
    if (window_.failed() && err) snprintf(err, 256, "engine run failed");
    if (recorder_) recorder_->Flush();
    last->first_game_digests.clear();
    for (auto& H : groups_)
      for (auto& g : H.games) last->first_game_digests.push_back(g->first_game_digest());
    last->reuse_added = reuse_->added();
    last->examples = recorder_ ? recorder_->examples() : 0;
    if (out) {
      const GameStats counted = window_.Fill(out);
      last->bias_pruned = counted.bias_entries_pruned;
      last->bias_adj = counted.bias_adj_abs_sum;
    }
    return window_.failed() ? 2 : 0;
  }

 private:
  struct PhaseCtl { std::atomic<bool> open{true}; std::atomic<int> loading{0}, delivered{0}; };

  // the request in feats[g] goes into the next free row of lane l's batch
  void LoadRequest(Group& H, Lane& L, int l, int g) {
    GameRunner& G = *H.games[g];
    const int slot = L.count.fetch_add(1);
    L.eval->Load(slot, H.feats[g]);
    if (dev_sym_) L.eval->SetSlotSymmetries(slot, G.BackMask());
    G.SetBackSlot(l, slot);
  }

  // Game g's task of a host phase of lane l, on the pool: the order is deliveries, then a straggler's pending load, then
  // TryAdvance.
  void AdvanceGame(Group& H, Lane& L, int l, int g, PhaseCtl& ctl, long phase_no) {
    GameRunner& G = *H.games[g];
    // the request in feats[g] goes into this lane's batch — while the phase is open; after that it waits for the next one
    auto load = [&]() -> bool {
      ctl.loading.fetch_add(1);
      const bool open = ctl.open.load();
      if (open) LoadRequest(H, L, l, g);
      else G.MarkUnloaded();
      ctl.loading.fetch_sub(1);
      return open;
    };
    for (int slot; (slot = G.FrontSlot(l)) >= 0;) {
      p3hip_result r;
      L.eval->Get(slot, r);
      G.DeliverResult(r);
    }
    ctl.delivered.fetch_add(1);     // this game no longer needs the lane's last results: the lane may run again
    // a request made by a straggler of the previous phase (after the deliveries: it must not pass for one of this
    // lane's last batch)
    const bool ok = !G.unloaded() || load();
    if (opt_.test_slow_us > 0 && ((uint64_t)g * 2654435761ull + (uint64_t)phase_no * 40503ull) % 61 == 0)   // tests: a slow game
      std::this_thread::sleep_for(std::chrono::microseconds(opt_.test_slow_us));
    if (ok && G.TryAdvance(&H.feats[g], depth_)) load();
    H.settled[g].store(1, std::memory_order_release);
  }

  // Wait for the games of a host phase — but not for a last few slow ones (an exact ladder read-out can take tens of
  // milliseconds) once another lane's run has come back, i.e. the GPU has nothing left to do: the batch then leaves
  // without them.
  void WaitOrHandOver(Group& H, const WorkerPool::JobRef& job, PhaseCtl& ctl, int cap) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      bool all_started = false;
      const int left = pool_.WaitFor(job, 100, &all_started);
      if (left == 0) break;
      if (left * 32 <= cap && all_started && ctl.delivered.load() == cap && H.waiting.load() > 0 &&
          std::chrono::steady_clock::now() - t0 >= std::chrono::milliseconds(1)) {
        ctl.open.store(false);
        while (ctl.loading.load() > 0) std::this_thread::yield();   // a load that saw the phase open completes
        H.late = job;
        ++H.handed_over_phases;
        H.handed_over_games += left;
        break;
      }
    }
  }

  // The second pass of a host phase: rows left empty (games that wait for a result of the other lane's batch, stragglers
  // handed over) go to games that can start another playout, so the batch stays full.
  void FillSpareRows(Group& H, Lane& L, int l, int cap) {
    std::atomic<int> spare{cap - L.count.load()};
    pool_.ParallelFor(cap, [this, &H, &L, &spare, l](int g) {
      if (!H.settled[g].load(std::memory_order_acquire)) return;   // a straggler: still at work on the pool
      GameRunner& G = *H.games[g];
      if (G.unloaded()) return;   // a straggler that has just ended with a request: feats[g] holds it for the next phase
      while (spare.load(std::memory_order_relaxed) > 0) {
        if (spare.fetch_sub(1) <= 0) { spare.fetch_add(1); break; }
        if (!G.TryAdvance(&H.feats[g], depth_)) { spare.fetch_add(1); break; }
        LoadRequest(H, L, l, g);
      }
    });
  }

  // The host phase of lane `l` of group H (the caller holds the group's turn): every game takes its results of
  // the lane's last run, in request order, and advances to its next leaf, which goes into the lane's next batch.
  // With several playouts in flight a game may have nothing to start (its next playout waits for a result of the
  // OTHER lane's batch): see FillSpareRows.
  void HostPhase(Group& H, Lane& L, int l) {
    const int cap = (int)H.games.size();
    // the previous phase's stragglers first: from here on nothing but this phase touches the group's games
    if (H.late) { pool_.Wait(H.late); H.late.reset(); }
    L.count.store(0);
    auto ctl = std::make_shared<PhaseCtl>();   // shared with the tasks: stragglers outlive the phase
    for (int g = 0; g < cap; ++g) H.settled[g].store(0, std::memory_order_relaxed);
    const long phase_no = H.phase_no++;
    WorkerPool::JobRef job = pool_.Submit(cap, [this, &H, &L, l, ctl, phase_no](int g) { AdvanceGame(H, L, l, g, *ctl, phase_no); });
    if (H.lanes.size() > 1) WaitOrHandOver(H, job, *ctl, cap);
    else pool_.Wait(job);
    if (depth_ > 1 && L.count.load() < cap) FillSpareRows(H, L, l, cap);
    // counters of the games whose tasks have ended (a straggler's are read when it has)
    for (int g = 0; g < cap; ++g)
      if (H.settled[g].load(std::memory_order_acquire)) {
        H.snap[g] = H.games[g]->stats();
        H.snap_past_opening[g] = H.games[g]->past_opening();
      }
  }

  // A lane's driver thread.  A batch = the lane's host phase (its turn among the group's lanes), then one engine run,
  // reported to the window; the lane leaves when the window says so.
  void LaneLoop(int h, int l) {
    Group& H = groups_[h];
    Lane& L = *H.lanes[l];
    for (;;) {
      {
        std::unique_lock<std::mutex> tl(H.turn_mu);
        H.waiting.fetch_add(1);
        H.turn_cv.wait(tl, [&] { return H.turn == l || H.quit; });
        H.waiting.fetch_sub(1);
        if (H.quit) break;
      }
      MeasureWindow::Run run;
      const auto a0 = std::chrono::steady_clock::now();
      HostPhase(H, L, l);
      {   // the counters as the host phase left them (games handed over as stragglers: as of their last settled phase)
        const GameStats now = H.Totals();
        run.delta = now - H.prev;
        H.prev = now;
        for (uint8_t po : H.snap_past_opening) run.past_opening += po;
        run.in_opening = run.past_opening < (long)H.games.size();
      }
      run.host_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - a0).count();
      if (phase_stats_)   // P3HOST_PHASE_STATS=1: how long the host phases take (a slow game holds up its whole group)
        ++phase_hist_[std::min(15, (int)(run.host_seconds * 1e3))];
      {
        std::lock_guard<std::mutex> tl(H.turn_mu);
        H.turn = (l + 1) % NL;
      }
      H.turn_cv.notify_all();
      run.start = std::chrono::steady_clock::now();
      run.ok = L.eval->Run();
      run.done = std::chrono::steady_clock::now();
      if (window_.Completed(h, l, run)) {
        {
          std::lock_guard<std::mutex> tl(H.turn_mu);
          H.quit = true;
        }
        H.turn_cv.notify_all();
        break;
      }
    }
  }

  const SelfPlayOptions opt_;
  const int NG, NL;
  const int depth_;        // playouts of one search in flight
  bool dev_sym_ = false;
  std::unique_ptr<ReuseBuffer> reuse_;
  std::unique_ptr<GameRecorder> recorder_;
  std::vector<Group> groups_;
  WorkerPool pool_;        // after the groups: its threads end before the games go away
  MeasureWindow window_;
  const bool phase_stats_;
  std::atomic<long> phase_hist_[16];
};

}  // namespace p3

using namespace p3;

namespace {
SelfPlayOptions g_options;     // written by the setters below, copied once at the top of a run
SelfPlayLastRun g_last_run;
}

extern "C" {

// Game-loop policy of subsequent p3host_selfplay_run calls: init_state_sampling = 0 plays
// every game from the empty board at komi 7.5 without forks (plumbing tests); otherwise the
// reference defaults (selfplay/main.cc:48-57) unless overridden here.
void p3host_selfplay_set_policy(int init_state_sampling, float use_seen_state_prob, float sel_mult_base,
                                float sel_mult_scale_factor) {
  g_options.init_state_sampling = init_state_sampling != 0;
  g_options.use_seen_state_prob = use_seen_state_prob;
  g_options.sel_mult_base = sel_mult_base;
  g_options.sel_mult_scale = sel_mult_scale_factor;
}
// --bias_cache_lambda / --bias_cache_alpha of subsequent runs (selfplay/main.cc:58-61,257-258;
// lambda 0 = off, the reference default; config/v4.json: 0.3 / 0.8).
void p3host_selfplay_set_bias_cache(float lambda, float alpha) {
  g_options.bias_cache_lambda = lambda;
  g_options.bias_cache_alpha = alpha;
}
// --sel_mult_calibration_file of subsequent runs (selfplay/main.cc:64-67,224); empty = built-in thresholds
void p3host_selfplay_set_calibration_file(const char* path) { g_options.calibration_file = path ? path : ""; }
// --early_stopping_enabled of subsequent runs (selfplay/main.cc:68,260; off by default)
void p3host_selfplay_set_early_stopping(int enabled) { g_options.early_stopping = enabled != 0; }
// Subsequent self-play runs over an engine library hand every leaf's random symmetry to the engine (an engine created
// with P3HIP_FLAG_SYMMETRY_SLOT and as many rows as slots) and neither rotate features nor results on the host; games,
// records and search results are the host path's.  Off by default; no effect on the null and hash evaluators.
void p3host_selfplay_set_device_symmetry(int enabled) { g_options.device_symmetry = enabled != 0; }
// Subsequent self-play runs over an engine library open the game groups' engines with P3HIP_FLAG_LAUNCH_GRAPH_ANY: a run of
// any size replays a captured graph from its third sighting on.  Off by default; no effect on the null and hash evaluators.
void p3host_selfplay_set_graph_any(int enabled) { g_options.graph_any = enabled != 0; }
// p3hip_graph_stats summed over the engines that the runs and matches since the last call opened and closed (engines with a
// launch-graph flag only): graphs held at the close, captures, replays, passes launched kernel by kernel, evictions
void p3host_graph_stats(uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = g_closed_graph_stats[i].exchange(0);
}
// bias-cache entries pruned / sum of |root adjustment| over the moves of the last run or game
long p3host_selfplay_last_bias_pruned() { return g_last_run.bias_pruned; }
double p3host_selfplay_last_bias_adj() { return g_last_run.bias_adj; }
// Number of game groups of subsequent p3host_selfplay_run calls (1..8).  Each group has its own
// engine instance and is either being advanced on the host or evaluated on the GPU; with G
// groups up to G - 1 forward passes are in flight while one group is on the host (one group:
// host and GPU alternate, BASELINE configs[2] as written).
void p3host_selfplay_set_groups(int n) { g_options.num_groups = n < 1 ? 1 : (n > 8 ? 8 : n); }
// Lanes per game group (engine instances whose batches the group's games fill in turn) and how many playouts of one
// search may wait for results at once.  1 / 1 (the default): host and GPU alternate within a group.  2 / up to 4:
// one group overlaps its host work with its own forward passes (BASELINE configs[2] as stated: 1024 games, batch 1024).
void p3host_selfplay_set_lanes(int lanes, int max_inflight) {
  g_options.num_lanes = lanes < 1 ? 1 : (lanes > 4 ? 4 : lanes);
  g_options.max_inflight = max_inflight < 1 ? 1 : (max_inflight > GumbelSearch::kMaxInflight ? GumbelSearch::kMaxInflight : max_inflight);
}
// > 0: subsequent p3host_selfplay_run calls measure exactly `batches` engine batches (bench.py's
// --steps), whichever groups they fall in, instead of running for `seconds`; 0 restores the time limit.
void p3host_selfplay_set_step_limit(long batches) { g_options.step_limit = batches > 0 ? batches : 0; }
// > 0 (takes precedence over the step limit): subsequent runs measure `rounds` ROUNDS.  The window opens at the
// completion of the warm-up batch of the group that finishes its warm-up last (the anchor) and closes at the
// completion of the anchor's `rounds`-th batch after that: both ends sit at the same phase of the groups' cycle on
// the GPU (the groups' forward passes complete in bursts, so a window between two arbitrary completions is off by
// up to a burst), and every batch of any group that completes inside (t0, t1] is counted — in steady state one per
// group and round.  bench.py's --steps; 0 = off.
void p3host_selfplay_set_step_rounds(long rounds) { g_options.step_rounds = rounds > 0 ? rounds : 0; }
// > 0: before the warm-up batches every group runs untimed batches until all its games have left
// their raw-policy opening (up to 30 moves of one evaluation each, self_play_thread.cc:44,363-366),
// at most `max_batches` of them, so that a short measured region is steady-state search; 0 = off.
void p3host_selfplay_set_advance_limit(int max_batches) { g_options.advance_limit = max_batches > 0 ? max_batches : 0; }
// reuse-buffer insertions and training examples written by the last p3host_selfplay_run
long p3host_selfplay_last_reuse_added() { return g_last_run.reuse_added; }
// tests: every 61st (game, host phase) pair sleeps `us` microseconds before it advances; 0 = off
void p3host_selfplay_set_test_slow_games(long us) { g_options.test_slow_us = us > 0 ? us : 0; }
// of the last p3host_selfplay_run: host phases that let their batch leave without a last few slow games, and those games
void p3host_selfplay_last_handed_over(long* phases, long* games) {
  if (phases) *phases = g_last_run.handed_over_phases;
  if (games) *games = g_last_run.handed_over_games;
}
// per game runner of the last p3host_selfplay_run (group by group): a digest of its first finished game, 0 if none
int p3host_selfplay_last_first_game_digests(uint64_t* out, int cap) {
  int n = 0;
  for (uint64_t d : g_last_run.first_game_digests)
    if (n < cap) out[n++] = d;
  return (int)g_last_run.first_game_digests.size();
}
long p3host_selfplay_last_examples() { return g_last_run.examples; }

// Enables game recording for subsequent p3host_selfplay_run calls (dir == "" disables):
// <dir>/sgf and <dir>/chunks as in selfplay/main.cc:157-158.
void p3host_selfplay_set_recorder(const char* dir, int gen, const char* worker_id, int flush_interval) {
  g_options.rec_dir = dir ? dir : "";
  g_options.rec_gen = gen;
  g_options.rec_worker = worker_id ? worker_id : "0";
  g_options.rec_flush_interval = flush_interval > 0 ? flush_interval : 128;
}

// Serializes a move list (encoded as in p3host_selfplay_one_game) the way the recorder does.
int p3host_sgf_from_moves(const int* moves, int n, float komi, int write_result, const char* b_name,
                          const char* w_name, char* out, int cap) {
  Game g(komi, true);
  for (int i = 0; i < n; ++i) {
    Color c = moves[i] > 0 ? kBlack : kWhite;
    int idx = (moves[i] > 0 ? moves[i] : -moves[i]) - 1;
    g.PlayMove(MoveLoc(idx), c);
  }
  if (write_result) g.WriteResult();
  std::string s = SgfGameString(g, b_name, w_name);
  if ((int)s.size() + 1 > cap) return -1;
  std::memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

// Runs self-play for about `seconds` (after `warmup_batches` unmeasured batches per group), or for the steps or rounds
// set before (measure_window.h).
// engine_lib: path of libp3hip.so, or NULL/"" for the NullEvaluator (uniform policy).
// Returns 0 on success; `err` (256 bytes) receives a message otherwise.
int p3host_selfplay_run(const char* engine_lib, const char* weights, int device, int num_games,
                        int num_threads, int default_n, int default_k, int selected_n,
                        int selected_k, int max_moves, double seconds, int warmup_batches,
                        uint64_t seed, p3host_selfplay_stats* out, char* err) {
  SelfPlayConfig cfg;
  cfg.default_n = default_n; cfg.default_k = default_k;
  cfg.selected_n = selected_n; cfg.selected_k = selected_k;
  cfg.max_moves = max_moves;
  SelfPlayJob job(g_options, num_threads, warmup_batches, seconds);   // the options of this run: copied here, once
  if (!job.Build(engine_lib, weights, device, num_games, cfg, seed, err)) return 1;
  job.Run();
  return job.Collect(&g_last_run, out, err);
}

// The reference's engine micro-benchmark, nn::Benchmark (cc/nn/engine/benchmark_engine.cc:77-108), over
// any library exporting the C ABI: 100 warm-up RunInference calls, then at most 1001 rounds (the
// reference's `num_inferences > 1000` bound) of LoadBatch x B -> RunInference -> GetBatch x B on ONE
// thread, the clock around RunInference only (its `elapsed_us`); `loop_seconds` is the whole timed loop,
// loads and gets included.  The reference walks a dataset that is not in its repository; here the
// rounds cycle through `n_feats` caller-supplied positions.  One difference, by design of the engine:
// this engine evaluates loaded slots only (the TRT engine always runs its static batch), so the batch is
// loaded once before the warm-up runs and they do the same work as the timed ones.
struct p3host_engine_benchmark_stats {
  long rounds, positions;
  double avg_run_us;        // mean of the per-round RunInference time (DefaultStats "avg_us")
  double loop_seconds;      // wall time of the timed loop: loads + runs + gets
  double checksum;          // sum over every fetched result of move_probs[argmax] (keeps the gets honest)
};
int p3host_engine_benchmark(const char* engine_lib, const char* weights, int device, int batch,
                            const p3hip_features* feats, int n_feats, int warmup_runs, int max_rounds,
                            p3host_engine_benchmark_stats* out, char* err) {
  if (!engine_lib || !engine_lib[0] || !feats || n_feats <= 0 || batch <= 0) {
    if (err) snprintf(err, 256, "engine_benchmark: engine library, positions and batch size are required");
    return 1;
  }
  HipEvaluator e;
  if (!e.Open(engine_lib, weights, batch, device)) {
    if (err) snprintf(err, 256, "%s", e.err.c_str());
    return 1;
  }
  for (int b = 0; b < batch; ++b) e.Load(b, feats[b % n_feats]);
  for (int i = 0; i < warmup_runs; ++i)
    if (!e.Run()) { if (err) snprintf(err, 256, "%s", e.err.c_str()); return 2; }
  p3hip_result r;
  double run_us = 0, checksum = 0;
  long rounds = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (; rounds < max_rounds; ++rounds) {
    const long off = rounds * (long)batch;
    for (int b = 0; b < batch; ++b) e.Load(b, feats[(off + b) % n_feats]);
    const auto s = std::chrono::steady_clock::now();
    if (!e.Run()) { if (err) snprintf(err, 256, "%s", e.err.c_str()); return 2; }
    run_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - s).count();
    for (int b = 0; b < batch; ++b) {
      e.Get(b, r);
      float best = r.move_probs[0];
      for (int i = 1; i < kNumMoves; ++i) best = std::max(best, r.move_probs[i]);
      checksum += best;
    }
  }
  if (out) {
    out->rounds = rounds;
    out->positions = rounds * (long)batch;
    out->avg_run_us = rounds ? run_us / rounds : 0;
    out->loop_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    out->checksum = checksum;
  }
  return 0;
}

// Plays ONE game to the end with the NullEvaluator or the HIP engine on a single thread and
// returns its move list (deterministic given the seed): plumbing test of BASELINE configs[0].
int p3host_selfplay_one_game(const char* engine_lib, const char* weights, int default_n, int default_k,
                             int max_moves, uint64_t seed, int* moves_out, int max_out, float* bscore,
                             float* wscore, long* evals, char* err) {
  SelfPlayConfig cfg;
  cfg.default_n = default_n; cfg.default_k = default_k;
  cfg.selected_n = default_n; cfg.selected_k = default_k;
  cfg.max_moves = max_moves;
  cfg.init_state_sampling = false;   // one empty-board game at komi 7.5
  cfg.bias_cache_lambda = g_options.bias_cache_lambda;
  cfg.bias_cache_alpha = g_options.bias_cache_alpha;
  std::unique_ptr<Evaluator> ev = MakeEvaluator(engine_lib, 0, err, [&](HipEvaluator& e) { return e.Open(engine_lib, weights, 1, 0); });
  if (!ev) return -1;
  GameRunner g(cfg, seed);
  p3hip_features f;
  p3hip_result r;
  while (g.stats().games == 0) {
    g.AdvanceToEval(&f);
    if (g.stats().games > 0) break;
    ev->Load(0, f);
    if (!ev->Run()) return -2;
    ev->Get(0, r);
    g.DeliverResult(r);
  }
  int n_out = 0;
  const std::vector<Move>& rec = g.last_moves();
  for (size_t i = Game::kMoveOffset; i < rec.size() && n_out < max_out; ++i)
    moves_out[n_out++] = (MoveIdx(rec[i].loc) + 1) * (rec[i].color == kBlack ? 1 : -1);
  if (bscore) *bscore = g.last_result().bscore;
  if (wscore) *wscore = g.last_result().wscore;
  if (evals) *evals = g.stats().evals;
  g_last_run.bias_pruned = g.stats().bias_entries_pruned;
  g_last_run.bias_adj = g.stats().bias_adj_abs_sum;
  return n_out;
}

// Test hook for the evaluation cache's reserve-then-fill protocol: `nreq` lookups over `nkeys` distinct keys,
// once in the one-at-a-time order (Find, on a miss Insert before the next lookup) and once with up to `depth`
// results outstanding (Probe, on a miss InsertPending at once and Fill `depth` - 1 lookups later).  Returns the
// number of lookups the two orders classify differently (hit / miss; a lookup that finds a reserved entry counts
// as the hit it would have been) or answer with a different result, plus 1000000 if the final contents differ.
long p3host_test_eval_cache_pipeline(int capacity, int nkeys, int nreq, int depth, uint64_t seed) {
  EvalCache seq(capacity), pipe(capacity);
  auto key_of = [](int k) {
    EvalCache::Key key{0x1234567ull * (uint64_t)(k + 1), {kNoopLoc, kNoopLoc, kNoopLoc, kNoopLoc, kNoopLoc}, 7.5f, kBlack};
    return key;
  };
  auto result_of = [](int k) {
    p3hip_result r;
    std::memset(&r, 0, sizeof r);
    r.err2_outcome = (float)k;
    return r;
  };
  struct Outstanding { uint64_t id; int key; int due; };
  std::deque<Outstanding> out;
  long diff = 0;
  uint64_t x = seed | 1;
  for (int i = 0; i < nreq; ++i) {
    while (!out.empty() && out.front().due <= i) {
      pipe.Fill(out.front().id, result_of(out.front().key));
      out.pop_front();
    }
    x = HashEvaluator::Mix(x);
    const int k = (int)(x % (uint64_t)nkeys);
    const p3hip_result* a = seq.Find(key_of(k));
    if (!a) seq.Insert(key_of(k), result_of(k));
    const p3hip_result* b = nullptr;
    uint64_t owner = 0;
    const EvalCache::Lookup lk = pipe.Probe(key_of(k), &b, &owner);
    if (lk == EvalCache::Lookup::kMiss) {
      const uint64_t id = pipe.InsertPending(key_of(k));
      out.push_back({id, k, i + 1 + (int)((x >> 20) % (uint64_t)depth)});
      std::stable_sort(out.begin(), out.end(), [](const Outstanding& p, const Outstanding& q) { return p.due < q.due; });
    }
    const bool hit_seq = a != nullptr, hit_pipe = lk != EvalCache::Lookup::kMiss;
    if (hit_seq != hit_pipe) ++diff;
    else if (a && a->err2_outcome != (float)k) ++diff;
    else if (lk == EvalCache::Lookup::kHit && b->err2_outcome != (float)k) ++diff;
    else if (lk == EvalCache::Lookup::kPending) {
      bool owned = false;
      for (const Outstanding& o : out) owned |= o.id == owner && o.key == k;
      if (!owned) ++diff;
    }
  }
  for (const Outstanding& o : out) pipe.Fill(o.id, result_of(o.key));
  for (int k = 0; k < nkeys; ++k) {   // same contents (these lookups stamp both caches alike)
    const p3hip_result* a = seq.Find(key_of(k));
    const p3hip_result* b = pipe.Find(key_of(k));
    if ((a != nullptr) != (b != nullptr) || (a && a->err2_outcome != b->err2_outcome)) return diff + 1000000;
  }
  return diff;
}

// Test hook for several playouts in flight (GameRunner::TryAdvance): plays `num_games` consecutive games of ONE
// game runner over the hash evaluator, with up to `depth` evaluation requests outstanding and the results handed
// back late — a result is delivered when nothing more can start, or earlier on a coin flip of `sched_seed`.
// out[0] = a digest of every finished game's moves and result, out[1] = evaluations, out[2] = cache hits,
// out[3] = moves, out[4] = the largest number of requests that were outstanding at once.
// depth 1 is the one-at-a-time order; every depth and every schedule must return the same out[0..3].
int p3host_test_game_inflight(int default_n, int default_k, int selected_n, int selected_k, int max_moves, uint64_t seed,
                              int depth, int num_games, int cache_entries, int init_state_sampling, int early_stopping,
                              uint64_t sched_seed, uint64_t* out) {
  SelfPlayConfig cfg;
  cfg.default_n = default_n; cfg.default_k = default_k;
  cfg.selected_n = selected_n; cfg.selected_k = selected_k;
  cfg.max_moves = max_moves;
  cfg.cache_entries_per_game = cache_entries;
  cfg.init_state_sampling = init_state_sampling != 0;
  cfg.early_stopping_enabled = early_stopping != 0;
  cfg.bias_cache_lambda = g_options.bias_cache_lambda;
  cfg.bias_cache_alpha = g_options.bias_cache_alpha;
  cfg.sel_mult_base = g_options.sel_mult_base;
  cfg.fork_params = ForkParams::ForReuse(g_options.use_seen_state_prob);
  auto reuse = std::make_unique<ReuseBuffer>(seed ^ 0x676f6578706c6f69ull);
  cfg.reuse = reuse.get();
  GameRunner g(cfg, seed);
  std::deque<p3hip_result> queue;   // results of the outstanding requests, oldest first
  uint64_t digest = 0xcbf29ce484222325ull, sched = sched_seed | 1, max_out = 0;
  long folded = 0;
  GameStats at_fold;   // counters when the last game finished (the next game's first request included, at every depth)
  auto fold = [&] {
    while (folded < g.stats().games) {   // (a finished game's record is replaced when the next one finishes)
      for (const Move& m : g.last_moves())
        digest = (digest ^ (uint64_t)(MoveIdx(m.loc) * 4 + (int)m.color + 2)) * 0x100000001b3ull;
      uint32_t bs, ws;
      const float b = g.last_result().bscore, w = g.last_result().wscore;
      std::memcpy(&bs, &b, 4);
      std::memcpy(&ws, &w, 4);
      digest = (digest ^ bs) * 0x100000001b3ull;
      digest = (digest ^ ws) * 0x100000001b3ull;
      ++folded;
      at_fold = g.stats();
    }
  };
  p3hip_features f;
  std::memset(&f, 0, sizeof f);   // FillFeatures writes every field; the hash also covers the padding
  while (g.stats().games < num_games) {
    sched = HashEvaluator::Mix(sched);
    const bool try_issue = queue.empty() || (sched & 3) != 0;
    if (try_issue && g.TryAdvance(&f, depth)) {
      queue.emplace_back();
      HashEvaluator::Evaluate(f, queue.back());
      max_out = std::max<uint64_t>(max_out, queue.size());
      fold();
      continue;
    }
    fold();
    if (queue.empty()) return 1;   // blocked with nothing outstanding: a scheduling bug
    g.DeliverResult(queue.front());
    queue.pop_front();
    fold();
  }
  out[0] = digest;
  out[1] = (uint64_t)at_fold.evals;
  out[2] = (uint64_t)at_fold.cache_hits;
  out[3] = (uint64_t)at_fold.moves;
  out[4] = max_out;
  return 0;
}

}  // extern "C"
