// eval_match.cc — the evaluation matches (cc/eval): the batching driver and the reference's thread-per-game one, the
// player-config entry points, the match summary, and the search test hooks that need a player's parameters.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>

#include "eval_match.h"
#include "evaluator.h"
#include "game_runner.h"   // EvalCache
#include "recorder.h"
#include "threaded_search.h"
#include "worker_pool.h"

using namespace p3;

namespace {
// The precision, latency and launch plan that a player's config asks of its engine.  SHARED_DEVICE: the two players'
// passes run concurrently.
uint32_t EvalEngineFlags(const EvalPlayerConfig& c) {
  return P3HIP_FLAG_SHARED_DEVICE | (c.nn_fp32 ? P3HIP_FLAG_FP32_ANY : 0u) | (c.nn_low_latency ? P3HIP_FLAG_LOW_LATENCY_ANY : 0u) |
         (c.nn_winograd ? P3HIP_FLAG_WINOGRAD : 0u) | (c.nn_graph_any ? P3HIP_FLAG_LAUNCH_GRAPH_ANY : 0u);
}

// The evaluator of an eval player (null for no engine library): a HIP engine opened with the plan flags of the
// player's config plus its symmetry flags.
// nn_symmetry_mask: the engine averages every evaluation over those symmetries; the host's random symmetry per
// leaf and its inverse stay, since the averaged result comes back in the orientation it was loaded in.
// nn_device_symmetry / nn_root_symmetry_mask: the engine rotates, a search's root visit under the root mask: a
// P3HIP_FLAG_SYMMETRY_SLOT engine of R = slots + 7 x games rows (a game has at most one root in flight; one copy per
// leaf without a root mask), at most 8 x slots.  Null with the message in `err`.
std::unique_ptr<Evaluator> MakeEvalEvaluator(const char* engine_lib, const char* weights, int slots, int games, int device,
                                             const EvalPlayerConfig& c, char* err) {
  return MakeEvaluator(engine_lib, 0, err, [&](HipEvaluator& h) {
    const uint32_t sym_mask = c.nn_symmetry_mask;
    const bool dev = c.device_symmetry();
    if (dev && sym_mask) {
      h.err = "nn_symmetry_mask cannot be combined with nn_device_symmetry / nn_root_symmetry_mask: an engine takes its "
              "symmetries either from its own mask or slot by slot";
      return false;
    }
    const uint32_t flags = EvalEngineFlags(c) | (sym_mask ? P3HIP_FLAG_SYMMETRY_AVG : 0u) | (dev ? P3HIP_FLAG_SYMMETRY_SLOT : 0u);
    const int rows = !dev ? 0 : c.nn_root_symmetry_mask ? std::min(8 * slots, slots + 7 * games) : slots;
    return h.Open(engine_lib, weights, slots, device, flags, rows) && (!sym_mask || h.SetSymmetries(sym_mask));
  });
}

// Under the p3host_parse_player_* entry points: parses the file and hands the config to `take`; 0, or 1 with the parser's
// message in `err`.
template <class Take>
int WithPlayerConfig(const char* path, char* err, Take&& take) {
  EvalPlayerConfig c;
  std::string e;
  if (!ParsePlayerConfig(path, &c, &e)) { if (err) snprintf(err, 256, "%s", e.c_str()); return 1; }
  take(c);
  return 0;
}
}  // namespace

extern "C" {

struct p3host_eval_stats {
  int games, cur_wins, cand_wins, draws, resignations;
  long moves, visits, collisions, positions, batches;
  double seconds;
  long cache_hits;                        // evaluations served by the NN cache (not in `positions`)
  float winrate, c95, rel_elo, elo_c95;   // cand's win rate +- 95 %, relative Elo +- (eval/main.cc:459-471)
};

// What the p3host_eval_set_* entry points set, for the matches after them; a match copies it once, at its top.
struct EvalOptions {
  int mode = 0, qfn = 2, nfn = 1, collision = 0, detector = 0;
  int descent = 0, mcgs = 0, cache_per_game = 256;
  float max_o = 1.0f, bias_lambda = 0.0f, bias_alpha = 0.8f;
  // per player (0 cur, 1 cand): the config file, and the --cur_* / --cand_* flags as "key: value" lines
  std::string config_file[2], cli[2];
  std::string recorder_dir, res_path;
};
static EvalOptions g_eval_options;
// Parallel-search knobs of subsequent p3host_eval_match calls (defaults = player_config.h:76-108:
// concurrent rounds, virtual_loss_soft, virtual_visit, abort, noop).
void p3host_eval_set_search(int mode, int q_fn, int n_fn, int collision, int detector) {
  EvalOptions& o = g_eval_options;
  o.mode = mode; o.qfn = q_fn; o.nfn = n_fn; o.collision = collision; o.detector = detector;
}
// descent policy (0 deterministic, 1 bu_uct + max_o_ratio), graph search, bias cache (lambda 0 = off)
// and NN-cache entries per game and player (--cache_size; 0 = off) of subsequent matches
void p3host_eval_set_search_ex(int descent, float max_o_ratio, int use_mcgs, float bias_lambda, float bias_alpha,
                               int cache_entries_per_game) {
  EvalOptions& o = g_eval_options;
  o.descent = descent; o.max_o = max_o_ratio; o.mcgs = use_mcgs;
  o.bias_lambda = bias_lambda; o.bias_alpha = bias_alpha;
  o.cache_per_game = cache_entries_per_game;
}
// --cur_config / --cand_config player files ("" = none), --recorder_path (SGFs of the games under
// <dir>/sgf; "" = none), --res_write_path (relative Elo; "" = none) of subsequent matches
void p3host_eval_set_paths(const char* cur_config, const char* cand_config, const char* recorder_dir,
                           const char* res_write_path) {
  EvalOptions& o = g_eval_options;
  o.config_file[0] = cur_config ? cur_config : "";
  o.config_file[1] = cand_config ? cand_config : "";
  o.recorder_dir = recorder_dir ? recorder_dir : "";
  o.res_path = res_write_path ? res_write_path : "";
}

void p3host_eval_set_player_flags(const char* cur, const char* cand) {
  g_eval_options.cli[0] = cur ? cur : "";
  g_eval_options.cli[1] = cand ? cand : "";
}

static bool MakeEvalPlayerConfigs(const EvalOptions& o, int visits_per_move, int leaves_per_round, EvalPlayerConfig pc[2],
                                  char* err) {
  EvalPlayerConfig base;
  base.n = visits_per_move;
  base.num_threads_per_game = leaves_per_round;
  base.search_mode = (SearchMode)o.mode;
  base.q_fn = (QFn)o.qfn;
  base.n_fn = (NFn)o.nfn;
  base.collision_policy = (CollisionPolicy)o.collision;
  base.collision_detector = (CollisionDetector)o.detector;
  base.descent_policy = (DescentPolicy)o.descent;
  base.max_o_ratio = o.max_o;
  base.use_mcgs = o.mcgs != 0;
  base.use_bias_cache = o.bias_lambda > 0.0f;
  base.bias_cache_lambda = o.bias_lambda;
  base.bias_cache_alpha = o.bias_alpha;
  pc[0] = pc[1] = base;
  static const char* const who[2] = {"cur", "cand"};
  std::string e;
  for (int p = 0; p < 2; ++p)
    if (!o.config_file[p].empty() && !ParsePlayerConfig(o.config_file[p], &pc[p], &e)) {
      if (err) snprintf(err, 256, "%s config: %s", who[p], e.c_str());
      return false;
    }
  // per-player command-line flags win over the file (eval/main.cc:146-246, 299-320)
  for (int p = 0; p < 2; ++p)
    if (!o.cli[p].empty() && !ApplyPlayerConfigText(o.cli[p], &pc[p], &e)) {
      if (err) snprintf(err, 256, "%s flags: %s", who[p], e.c_str());
      return false;
    }
  return true;
}

// match bookkeeping shared by both drivers: results, Elo, result file, SGF batch
struct EvalGameOutcome { int cur_result; bool resigned; Color winner; std::string sgf; };
static void FinishEvalMatch(const EvalOptions& o, const std::vector<EvalGameOutcome>& games, p3host_eval_stats* out) {
  for (const auto& g : games) {
    out->cur_wins += g.cur_result > 0;
    out->cand_wins += g.cur_result < 0;
    out->draws += g.cur_result == 0;
    out->resignations += g.resigned;
  }
  out->games = (int)games.size();
  const MatchSummary m = SummarizeMatch(out->cand_wins, out->games);
  out->winrate = m.winrate; out->c95 = m.c95; out->rel_elo = m.rel_elo; out->elo_c95 = m.elo_c95;
  if (!o.res_path.empty()) WriteMatchResult(o.res_path, m.rel_elo);
  if (!o.recorder_dir.empty()) {   // GameRecorder::Create(recorder_path, ..., "EVAL_<cur>_<cand>"), eval/main.cc:418-422
    ::mkdir(o.recorder_dir.c_str(), 0755);
    ::mkdir((o.recorder_dir + "/sgf").c_str(), 0755);
    SgfRecorder rec(o.recorder_dir + "/sgf", 0, "EVAL_cur_cand");
    for (const auto& g : games) rec.RecordGame(g.sgf);
    rec.Flush();
  }
}
static std::string EvalGameSgf(const Game& game, bool cur_is_black, bool resigned, Color winner) {
  Game::Result r = game.result();
  if (resigned) { r = Game::Result(); r.winner = winner; r.by_resign = true; }
  return SgfGameString(game.komi(), r, game.moves(), Game::kMoveOffset, cur_is_black ? "cur" : "cand",
                       cur_is_black ? "cand" : "cur");
}

// Evaluation-match drivers: keep the NN cache in the engine's HBM table (p3hip_cache_*, 2^log2_entries entries per
// engine: one table for all games and workers of a player) — instead of NNInterface's per-thread host LRUs in the
// thread-per-game driver, behind the per-game host caches in the batching one; 0 = host caches only (the reference's
// arrangement).
static std::atomic<int> g_device_nn_cache_log2{0};
static std::atomic<long> g_device_nn_cache_hits{0}, g_device_nn_cache_lookups{0};
void p3host_set_device_nn_cache(int log2_entries) { g_device_nn_cache_log2.store(log2_entries < 0 ? 0 : log2_entries); }
long p3host_device_nn_cache_hits() { return g_device_nn_cache_hits.load(); }   // of the last thread-per-game match
long p3host_device_nn_cache_lookups() { return g_device_nn_cache_lookups.load(); }

// The batching match driver: `num_games` evaluation games between two networks with the batch parallel search
// (eval.cc:103-518).  One engine instance per player, batch = num_games * leaves_per_round slots; every game keeps an NN
// cache per player (NNKey with five last moves, nn_interface.cc:92-132), so a position the search reaches again — in a
// later move's search, or through the other player's tree — costs no slot.
class EvalMatchJob {
 public:
  EvalMatchJob(const EvalOptions& opt, const EvalPlayerConfig pc[2], int num_games, int max_moves, int num_threads, uint64_t seed)
      : num_games(num_games), slots(num_games * std::max(pc[0].num_threads_per_game, pc[1].num_threads_per_game)),
        pool(num_threads > 0 ? num_threads : 1), want(num_games, 0), base(num_games, 0), need(num_games, 0),
        eng_of(num_games, -1), slot_of(num_games), key_of(num_games), hit_of(num_games), feats(2 * (size_t)slots) {
    for (int g = 0; g < num_games; ++g)
      games.emplace_back(new EvalGame(g, pc[0], pc[1], max_moves, seed * 0x9E3779B97F4A7C15ull + (uint64_t)g * 0xBF58476D1CE4E5B9ull));
    for (int g = 0; g < 2 * num_games; ++g) caches.emplace_back(opt.cache_per_game, 5);
  }

  // The two players' evaluators (engine_lib NULL/"" = NullEvaluator for both), with the on-device NN cache if it is on.
  // False with a message in `err`.
  bool Open(const char* engine_lib, const char* const weights[2], int device, const EvalPlayerConfig pc[2], char* err) {
    for (int e = 0; e < 2; ++e) {
      ev[e] = MakeEvalEvaluator(engine_lib, weights[e], slots, num_games, device, pc[e], err);
      if (!ev[e]) return false;
    }
    const int dc_log2 = g_device_nn_cache_log2.load();
    if (dc_log2 > 0 && engine_lib && engine_lib[0]) {
      device_cache = ev[0]->EnableDeviceCache(dc_log2) && ev[1]->EnableDeviceCache(dc_log2);
      if (!device_cache) {
        if (err) snprintf(err, 256, "the engine has no on-device NN cache (p3hip_cache_enable)");
        return false;
      }
    }
    return true;
  }

  // Plays the games to their ends.  False: an engine run failed.
  bool Play() {
    t0 = std::chrono::steady_clock::now();
    pool.ParallelFor(num_games, [this](int g) { Advance(g); });
    for (;;) {
      // Every game wants leaves from the engine of its side to move: fill both engines' batches,
      // run the two forward passes CONCURRENTLY (own streams on the same device), hand back.
      int total[2] = {0, 0};
      for (int g = 0; g < num_games; ++g) {
        base[g] = -1;
        eng_of[g] = -1;
        if (want[g] <= 0) continue;
        const int e = games[g]->active_engine();
        eng_of[g] = e;
        base[g] = total[e];
        total[e] += need[g];
      }
      if (total[0] + total[1] == 0) return true;
      pool.ParallelFor(num_games, [this](int g) { Load(g); });
      bool ok[2] = {true, true};
      std::thread second;
      if (total[1] > 0) second = std::thread([&] { ok[1] = ev[1]->Run(); });
      if (total[0] > 0) ok[0] = ev[0]->Run();
      if (second.joinable()) second.join();
      if (!ok[0] || !ok[1]) return false;
      positions += total[0] + total[1];
      batches += (total[0] > 0) + (total[1] > 0);
      pool.ParallelFor(num_games, [this](int g) { Deliver(g); });
    }
  }

  void Collect(const EvalOptions& opt, p3host_eval_stats* out) {
    std::memset(out, 0, sizeof *out);
    std::vector<EvalGameOutcome> outcomes;
    for (auto& g : games) {
      outcomes.push_back({g->cur_result(), g->resigned(), g->winner(),
                          EvalGameSgf(g->game(), g->cur_is_black(), g->resigned(), g->winner())});
      out->moves += g->num_moves();
      out->visits += g->visits();
      out->collisions += g->collisions();
    }
    FinishEvalMatch(opt, outcomes, out);
    out->positions = positions;
    out->batches = batches;
    out->cache_hits = cache_hits.load();
    g_device_nn_cache_hits.store(device_hits.load());
    g_device_nn_cache_lookups.store(device_lookups.load());
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }

 private:
  // Advances game g until it wants evaluations the cache cannot answer (or has finished).
  void Advance(int g) {
  for (;;) {
    want[g] = games[g]->Step();
    need[g] = 0;
    if (want[g] <= 0) return;
    const int e = games[g]->active_engine();
    EvalCache& cache = caches[2 * g + e];
    slot_of[g].assign(want[g], -1);
    key_of[g].resize(want[g]);
    if ((int)hit_of[g].size() < want[g]) hit_of[g].resize(want[g]);
    for (int i = 0; i < want[g]; ++i) {
      key_of[g][i] = cache.MakeKey(games[g]->eval_position(i), games[g]->eval_color_of(i));
      if (const p3hip_result* hit = cache.Find(key_of[g][i])) hit_of[g][i] = *hit;
      else slot_of[g][i] = need[g]++;
    }
    if (need[g] > 0) return;
    for (int i = 0; i < want[g]; ++i) games[g]->DeliverCached(i, hit_of[g][i]);   // all cached
    cache_hits.fetch_add(want[g], std::memory_order_relaxed);
  }
  }
  // Game g's evaluations that the cache did not answer go into its engine's batch.
  void Load(int g) {
    if (base[g] < 0) return;
    const int e = eng_of[g];
    p3hip_features* f = &feats[(size_t)e * slots + base[g]];
    for (int i = 0; i < want[g]; ++i) {
      if (slot_of[g][i] < 0) continue;
      games[g]->FillEval(i, f + slot_of[g][i]);
      if (device_cache) {
        uint64_t lo, hi;
        EvalCache::Digest(key_of[g][i], &lo, &hi);
        ev[e]->LoadKeyed(base[g] + slot_of[g][i], f[slot_of[g][i]], lo, hi, (int)games[g]->eval_symmetry(i));
      } else {
        ev[e]->Load(base[g] + slot_of[g][i], f[slot_of[g][i]]);
      }
      if (const uint32_t mask = games[g]->eval_mask(i)) ev[e]->SetSlotSymmetries(base[g] + slot_of[g][i], mask);
    }
  }
  // Game g takes its results (cached ones included), stores the new ones, and advances.
  void Deliver(int g) {
    if (base[g] < 0) return;
    const int e = eng_of[g];
    EvalCache& cache = caches[2 * g + e];
    p3hip_result r;
    for (int i = 0; i < want[g]; ++i) {
      if (slot_of[g][i] < 0) {
        games[g]->DeliverCached(i, hit_of[g][i]);
        cache_hits.fetch_add(1, std::memory_order_relaxed);
        continue;
      }
      if (device_cache) {
        int sym = (int)games[g]->eval_symmetry(i);
        bool hit = false;
        ev[e]->GetKeyed(base[g] + slot_of[g][i], r, &sym, &hit);
        device_lookups.fetch_add(1, std::memory_order_relaxed);
        if (hit) device_hits.fetch_add(1, std::memory_order_relaxed);
        games[g]->DeliverUnder(i, r, (Symmetry)sym);   // un-symmetrises by the symmetry of the stored result
      } else {
        ev[e]->Get(base[g] + slot_of[g][i], r);
        games[g]->Deliver(i, r);   // un-symmetrises r in place
      }
      cache.Insert(key_of[g][i], r);
    }
    Advance(g);
  }

  const int num_games, slots;
  std::unique_ptr<Evaluator> ev[2];
  bool device_cache = false;
  std::atomic<long> device_lookups{0}, device_hits{0};
  std::vector<std::unique_ptr<EvalGame>> games;
  std::vector<EvalCache> caches;   // [game * 2 + engine]
  WorkerPool pool;
  std::vector<int> want, base, need, eng_of;
  std::vector<std::vector<int>> slot_of;          // evaluation i of game g -> engine slot offset, -1 = cached
  std::vector<std::vector<EvalCache::Key>> key_of;
  // copies of the cached results found in Advance(): the deliveries interleave with Insert(),
  // which may evict the very entry a later evaluation of the same round hit (cache smaller than a round)
  std::vector<std::vector<p3hip_result>> hit_of;
  std::vector<p3hip_features> feats;
  long positions = 0, batches = 0;
  std::atomic<long> cache_hits{0};
  std::chrono::steady_clock::time_point t0;
};

int p3host_eval_match(const char* engine_lib, const char* cur_weights, const char* cand_weights, int device,
                      int num_games, int visits_per_move, int leaves_per_round, int max_moves, int num_threads,
                      uint64_t seed, p3host_eval_stats* out, char* err) {
  const EvalOptions opt = g_eval_options;   // the options of this match
  EvalPlayerConfig pc[2];
  if (!MakeEvalPlayerConfigs(opt, visits_per_move, leaves_per_round, pc, err)) return 3;
  EvalMatchJob job(opt, pc, num_games, max_moves, num_threads, seed);
  const char* const weights[2] = {cur_weights, cand_weights};
  if (!job.Open(engine_lib, weights, device, pc, err)) return 1;
  if (!job.Play()) {
    if (err) snprintf(err, 256, "engine run failed");
    return 2;
  }
  if (out) job.Collect(opt, out);
  return 0;
}

// One game of the thread-per-game match, on its own thread (PlayEvalGame, eval.cc:103-518)
struct ThreadedGameResult { EvalGameOutcome outcome; long moves = 0, visits = 0, collisions = 0; };
static void PlayThreadedEvalGame(int g, const EvalPlayerConfig pc[2], std::unique_ptr<NNInterface> nn[2], int max_moves,
                                 uint64_t seed, ThreadedGameResult* out) {
  Probability prob(seed * 0x9E3779B97F4A7C15ull + (uint64_t)g * 0xBF58476D1CE4E5B9ull);
  const bool cur_is_black = g % 2 == 0;
  const int player_of[2] = {cur_is_black ? 0 : 1, cur_is_black ? 1 : 0};   // colour index (0 black) -> player
  Game game(7.5f, true);
  std::unique_ptr<BiasCache> bias[2];
  NodePool pool[2];
  TreeNode* tree[2];
  std::unique_ptr<ThreadedSearch> search[2];
  for (int s = 0; s < 2; ++s) {
    const EvalPlayerConfig& c = pc[player_of[s]];
    pool[s].set_graph(c.use_mcgs);
    if (c.use_bias_cache) bias[s].reset(new BiasCache(c.bias_cache_alpha, c.bias_cache_lambda));
    tree[s] = pool[s].GetOrCreate(game.board().hash(), kBlack, false);
    search[s].reset(new ThreadedSearch(nn[player_of[s]]->MakeSlot(g * c.num_threads_per_game), bias[s].get()));
  }
  Color color = kBlack, resigned = kEmpty;
  while (!game.IsGameOver() && game.num_moves() < max_moves) {
    const int s = color == kBlack ? 0 : 1;
    const EvalPlayerConfig& c = pc[player_of[s]];
    ThreadedSearch::Params p;
    p.num_threads = c.num_threads_per_game;
    p.total_visit_budget = c.time_ms > 0 ? (1 << 30) : c.n;
    p.total_visit_time_ms = c.time_ms;
    p.puct = MakeSearchPuctParams(c);
    p.score_util = MakeScoreUtility(c);
    p.fns = VirtualFns{c.q_fn, c.n_fn, c.vl_delta};
    p.descent = c.descent_policy;
    p.collision = c.collision_policy;
    p.detector = c.collision_detector;
    p.max_collision_retries = c.max_collision_retries;
    p.max_o_ratio = c.max_o_ratio;
    const ThreadedSearch::Result r = search[s]->Run(prob, game, &pool[s], tree[s], color, p);
    out->visits += r.num_visits;
    out->collisions += r.num_collisions;
    if (VOutcome(tree[s]) < kResignThreshold) { resigned = color; break; }   // eval.cc:277-282
    game.PlayMove(r.move, color);
    color = Opp(color);
    for (int t = 0; t < 2; ++t) {   // both trees follow the move, eval.cc:318-352
      TreeNode* next = tree[t]->child(MoveIdx(r.move));
      if (!next) next = pool[t].GetOrCreate(game.board().hash(), color, game.IsGameOver());
      pool[t].Reap(next);
      tree[t] = next;
      if (bias[t]) bias[t]->PruneUnused();
    }
  }
  // a finished game leaves both interfaces' signalling quorum (eval.cc:505-507)
  for (int s = 0; s < 2; ++s) nn[s]->MakeSlot(0).UnregisterSearchTask();
  Color winner;
  if (resigned != kEmpty) {
    winner = Opp(resigned);
  } else {
    game.WriteResult();
    winner = game.result().winner;
  }
  const int cur_result = winner == kEmpty ? 0 : ((winner == kBlack) == cur_is_black ? 1 : -1);
  out->outcome = {cur_result, resigned != kEmpty, winner, EvalGameSgf(game, cur_is_black, resigned != kEmpty, winner)};
  out->moves = game.num_moves();
}

// The reference's own shape of the match (eval/main.cc:380-452, eval.cc:103-518): one OS thread
// per game, each player's engine behind its own NNInterface with kExplicit signalling,
// num_shared_search_tasks = num_games, batch = num_games * threads_per_game slots and the
// per-thread NN cache on (cache_size entries in total per interface), the side to move running
// the threaded mcts::Search (threaded_search.h) on slot range [game * T, (game + 1) * T).
int p3host_eval_match_threads(const char* engine_lib, const char* cur_weights, const char* cand_weights, int device,
                              int num_games, int visits_per_move, int threads_per_game, int max_moves,
                              long cache_size, uint64_t seed, p3host_eval_stats* out, char* err) {
  const EvalOptions opt = g_eval_options;   // the options of this match
  EvalPlayerConfig pc[2];
  if (!MakeEvalPlayerConfigs(opt, visits_per_move, threads_per_game, pc, err)) return 3;
  const bool use_null = !engine_lib || !engine_lib[0];
  std::unique_ptr<NNInterface> nn[2];
  for (int e = 0; e < 2; ++e) {
    const int batch = num_games * pc[e].num_threads_per_game;
    std::unique_ptr<Evaluator> ev = MakeEvalEvaluator(engine_lib, e == 0 ? cur_weights : cand_weights, batch, num_games, device, pc[e], err);
    if (!ev) return 1;
    nn[e].reset(new NNInterface(batch, NNInterface::kTimeoutUs, (size_t)cache_size, std::move(ev),
                                NNInterface::SignalKind::kExplicit, num_games));
    if (!use_null && pc[e].device_symmetry() &&
        (!nn[e]->SetDeviceSymmetry(true) || !nn[e]->SetRootSymmetryMask(pc[e].nn_root_symmetry_mask))) {
      if (err) snprintf(err, 256, "the engine has no per-slot symmetries (p3hip_set_slot_symmetries)");
      return 1;
    }
    const int dc = g_device_nn_cache_log2.load();
    if (dc > 0 && !use_null && !nn[e]->EnableDeviceCache(dc)) {
      if (err) snprintf(err, 256, "the engine has no on-device NN cache (p3hip_cache_enable)");
      return 1;
    }
  }
  std::vector<ThreadedGameResult> results(num_games);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> threads;
  for (int g = 0; g < num_games; ++g)
    threads.emplace_back([&, g] { PlayThreadedEvalGame(g, pc, nn, max_moves, seed, &results[g]); });
  for (auto& t : threads) t.join();
  g_device_nn_cache_hits.store(nn[0]->device_cache_hits() + nn[1]->device_cache_hits());
  g_device_nn_cache_lookups.store(nn[0]->device_cache_lookups() + nn[1]->device_cache_lookups());
  if (out) {
    std::memset(out, 0, sizeof *out);
    std::vector<EvalGameOutcome> outcomes;
    for (const ThreadedGameResult& r : results) {
      outcomes.push_back(r.outcome);
      out->moves += r.moves; out->visits += r.visits; out->collisions += r.collisions;
    }
    FinishEvalMatch(opt, outcomes, out);
    out->batches = nn[0]->num_inferences() + nn[1]->num_inferences();
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  return 0;
}

// core::RelativeElo / the match summary, for the tests
void p3host_match_summary(int num_cand_won, int num_games, float* out4) {
  const MatchSummary m = SummarizeMatch(num_cand_won, num_games);
  out4[0] = m.winrate; out4[1] = m.c95; out4[2] = m.rel_elo; out4[3] = m.elo_c95;
}
// parses a player config file; returns 0 and fills out[0..39] with its fields (order below), or 1 with a message
int p3host_parse_player_config(const char* path, float* out, char* err) {
  return WithPlayerConfig(path, err, [&](const EvalPlayerConfig& c) {
    const PuctParams sp = MakeSearchPuctParams(c), rp = MakeRootPuctParams(c);
    const ScoreUtilityParams su = MakeScoreUtility(c);
    const float v[40] = {(float)c.n, (float)c.num_threads_per_game, c.c_puct, c.c_puct_visit_scaling, c.root_fpu,
                         (float)c.var_scale_cpuct, (float)(int)c.q_fn, (float)(int)c.n_fn, (float)(int)c.collision_policy,
                         (float)(int)c.collision_detector, (float)(int)c.search_mode, (float)(int)c.descent_policy,
                         c.max_o_ratio, (float)c.use_mcgs, (float)c.use_bias_cache, (float)c.time_ms,
                         // 16..
                         (float)c.k, c.noise_scaling, (float)c.early_stopping_for_gumbel, (float)c.use_puct,
                         (float)c.use_puct_v, c.c_puct_v_2, c.tau, (float)c.use_lcb, c.score_weight, (float)(int)su.mode,
                         // 26..
                         (float)c.enable_m3_bonus, (float)c.var_scale_prior_visits, (float)c.m3_prior_visits, c.p_opt_weight,
                         (float)c.enable_pondering, (float)c.time_control_flags, c.vl_delta, (float)c.max_collision_retries,
                         // 34..: derived parameters
                         (float)(int)sp.kind, (float)(int)rp.kind, rp.c_puct_visit_scaling, rp.tau, (float)UsesParallelSearch(c),
                         c.bias_cache_alpha};
    std::memcpy(out, v, sizeof v);
  });
}
// Single keys of a player config file (tests), each 0 and the value, or 1 with the parser's message: nn_symmetry_mask;
// nn_device_symmetry (what the player gets, the root mask implying it) and nn_root_symmetry_mask; nn_fp32; nn_low_latency;
// nn_winograd; nn_graph_any
int p3host_parse_player_symmetry_mask(const char* path, uint32_t* mask, char* err) {
  return WithPlayerConfig(path, err, [&](const EvalPlayerConfig& c) { *mask = c.nn_symmetry_mask; });
}
int p3host_parse_player_device_symmetry(const char* path, int* device_symmetry, uint32_t* root_mask, char* err) {
  return WithPlayerConfig(path, err, [&](const EvalPlayerConfig& c) {
    *device_symmetry = c.device_symmetry() ? 1 : 0;
    *root_mask = c.nn_root_symmetry_mask;
  });
}
int p3host_parse_player_fp32(const char* path, int* fp32, char* err) {
  return WithPlayerConfig(path, err, [&](const EvalPlayerConfig& c) { *fp32 = c.nn_fp32; });
}
int p3host_parse_player_low_latency(const char* path, int* low_latency, char* err) {
  return WithPlayerConfig(path, err, [&](const EvalPlayerConfig& c) { *low_latency = c.nn_low_latency; });
}
int p3host_parse_player_winograd(const char* path, int* winograd, char* err) {
  return WithPlayerConfig(path, err, [&](const EvalPlayerConfig& c) { *winograd = c.nn_winograd; });
}
int p3host_parse_player_graph_any(const char* path, int* graph_any, char* err) {
  return WithPlayerConfig(path, err, [&](const EvalPlayerConfig& c) { *graph_any = c.nn_graph_any; });
}

// PuctScorer::ComputeScores on a hand-built node (tests): children given as (action, visits, v, v_var, v_m3,
// n_in_flight); pp = {c_puct, c_puct_visit_scaling, c_puct_v_2, use_puct_v, enable_var_scaling,
// var_scale_prior_visits, enable_m3_bonus, m3_prior_visits, p_opt_weight, root_fpu}; fns = {q_fn, n_fn, vl_delta}
void p3host_test_puct_scores(int node_n, float node_v, float node_v_var, const float* move_probs, const float* opt_probs,
                             int n_children, const int* actions, const int* visits, const float* child_v,
                             const float* child_v_var, const double* child_v_m3, const int* in_flight,
                             const float* ppv, const float* fns, int is_root, float* scores) {
  NodePool pool;
  TreeNode* node = pool.Create();
  node->n = node_n; node->v = node_v; node->v_var = node_v_var;
  std::memcpy(node->move_probs, move_probs, sizeof node->move_probs);
  std::memcpy(node->opt_probs, opt_probs, sizeof node->opt_probs);
  for (int i = 0; i < n_children; ++i) {
    TreeNode* ch = pool.Create();
    ch->v = child_v[i]; ch->v_var = child_v_var[i]; ch->v_m3 = child_v_m3[i];
    ch->n_in_flight = in_flight[i];
    node->children.push_back(ChildEdge{(int16_t)actions[i], visits[i], ch});
  }
  PuctParams pp;
  pp.c_puct = ppv[0]; pp.c_puct_visit_scaling = ppv[1]; pp.c_puct_v_2 = ppv[2]; pp.use_puct_v = ppv[3] != 0;
  pp.enable_var_scaling = ppv[4] != 0; pp.var_scale_prior_visits = (int)ppv[5]; pp.enable_m3_bonus = ppv[6] != 0;
  pp.m3_prior_visits = (int)ppv[7]; pp.p_opt_weight = ppv[8]; pp.root_fpu = ppv[9];
  const VirtualFns vf{(QFn)(int)fns[0], (NFn)(int)fns[1], fns[2]};
  PuctScoresAll(node, pp, is_root != 0, scores, vf);
}

// LeafEvaluator::EvaluateLeaf on a neutral evaluation (value 0, expected score 0), the situation of
// cc/mcts/__tests__/leaf_evaluator_test.cc: returns init_util_est
float p3host_test_evaluate_leaf(int color_to_move, int root_color, float root_score_est, int integral, float score_weight) {
  p3hip_result r;
  std::memset(&r, 0, sizeof r);
  r.value_probs[0] = r.value_probs[1] = 0.5f;
  r.score_probs[399] = r.score_probs[400] = 0.5f;   // E[score] = 0
  NodePool pool;
  TreeNode* node = pool.Create();
  EvaluateLeaf(r, node, (Color)color_to_move, (Color)root_color, root_score_est,
               ScoreUtilityParams{score_weight, integral ? ScoreUtilityMode::kIntegral : ScoreUtilityMode::kDirect});
  return node->init_util_est;
}

// LeafEvaluator::ScoreUtility (leaf_evaluator.cc:125-132)
float p3host_test_score_utility(int integral, float score_weight, float score_est, float score_stddev, float root_score_est) {
  return ScoreUtility(ScoreUtilityParams{score_weight, integral ? ScoreUtilityMode::kIntegral : ScoreUtilityMode::kDirect},
                      score_est, score_stddev, root_score_est);
}

}  // extern "C"
