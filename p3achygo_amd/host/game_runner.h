// game_runner.h — one self-play game as a resumable state machine, with what it owns: the recorder of finished games,
// the game-loop configuration, the per-game evaluation cache.
//
// Game loop restated from selfplay::Run (cc/selfplay/self_play_thread.cc:309-920), core part:
// raw-policy opening moves, playout-cap randomisation (full search with probability 0.25,
// otherwise a fast search with per-game k and noise scaling), temperature schedule, Gumbel
// root search, tree reuse + Reap, pass-alive refresh at moves 200/250/.../400, max_moves,
// final scoring, init-state sampling (handicap games, GoExploit restarts), the fork manager,
// down-bad visit annealing, sel_mult, the per-game bias cache (--bias_cache_lambda/alpha, on in
// config/v4.json) and the recorders.  Not restated: the opening book
// (probability 0 in the reference).
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "evaluator.h"
#include "features.h"
#include "game_stats.h"
#include "recorder.h"
#include "search.h"
#include "selfplay_policy.h"
#include "tf_recorder.h"

namespace p3 {

// ---- one game ----------------------------------------------------------------------------
// Buffers finished games for both recorders (recorder::GameRecorder, game_recorder.cc:68-175):
// SGF lines only for games that started on an empty board, training examples for all.
class GameRecorder {
 public:
  GameRecorder(const std::string& path, int gen, const std::string& worker_id, int flush_interval)
      : sgf_(path + "/sgf", gen, worker_id), tf_(path + "/chunks", gen, worker_id), flush_interval_(flush_interval) {
    io_ = std::thread([this] { IoLoop(); });   // game_recorder.cc:83: flushes run on an IO thread
  }
  ~GameRecorder() {
    {
      std::lock_guard<std::mutex> l(mu_);
      quit_ = true;
    }
    cv_.notify_all();
    io_.join();
  }
  void RecordGame(const Board& init_board, const Game& game, std::vector<MoveSearchRecord> infos) {
    if (init_board.IsEmpty()) sgf_.RecordGame(SgfGameString(game, "p3achygo", "p3achygo"));   // game_recorder.cc:20,101-108
    std::lock_guard<std::mutex> l(mu_);
    tf_.RecordGame(init_board, game, std::move(infos));
    if (++buffered_ >= flush_interval_ && !flushing_) {   // should_flush_, game_recorder.cc:113-115
      want_flush_ = true;
      cv_.notify_all();
    }
  }
  // Final flush (the reference flushes on exit): waits for the IO thread, then writes the rest.
  void Flush() {
    std::unique_lock<std::mutex> l(mu_);
    cv_.wait(l, [this] { return !flushing_ && !want_flush_; });
    auto recs = tf_.TakeRecords();
    buffered_ = 0;
    l.unlock();
    sgf_.Flush();
    const int n = tf_.FlushRecords(std::move(recs));
    l.lock();
    examples_ += n;
  }
  long examples() {
    std::lock_guard<std::mutex> l(mu_);
    return examples_;
  }

 private:
  // Unlike the reference (which holds every game thread's mutex while it replays the games,
  // game_recorder.cc:158-175) the buffered games are detached under the lock and written
  // outside it: no game waits for a flush.
  void IoLoop() {
    std::unique_lock<std::mutex> l(mu_);
    for (;;) {
      cv_.wait(l, [this] { return want_flush_ || quit_; });
      if (quit_) return;
      want_flush_ = false;
      flushing_ = true;
      auto recs = tf_.TakeRecords();
      buffered_ = 0;
      l.unlock();
      sgf_.Flush();
      const int n = tf_.FlushRecords(std::move(recs));
      l.lock();
      examples_ += n;
      flushing_ = false;
      cv_.notify_all();
    }
  }

  SgfRecorder sgf_;
  TfRecorder tf_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::thread io_;
  int flush_interval_, buffered_ = 0;
  bool want_flush_ = false, flushing_ = false, quit_ = false;
  long examples_ = 0;
};

struct SelfPlayConfig {       // SPConfig, cc/selfplay/self_play_thread.h:38-61
  int selected_n = 128, selected_k = 8;   // --gumbel_selected_{n,k}  selfplay/main.cc:40-43
  int default_n = 32, default_k = 5;      // --gumbel_default_{n,k}   selfplay/main.cc:44-47
  int max_moves = 600;                    // --max_moves
  int nonroot_var_scale_prior_visits = 10;
  float bias_cache_lambda = 0.0f, bias_cache_alpha = 0.8f;   // --bias_cache_{lambda,alpha} main.cc:58-61 (0 = off)
  bool early_stopping_enabled = false;                       // --early_stopping_enabled main.cc:68
  // the engine rotates (P3HIP_FLAG_SYMMETRY_SLOT): features go out un-rotated, the request's random symmetry travels as
  // the slot's mask (GameRunner::BackMask), results come back in the game's orientation
  bool device_symmetry = false;
  float use_seen_state_prob = 0.5f;       // --use_seen_state_prob     main.cc:48-50
  float sel_mult_base = 0.0f, sel_mult_scale_factor = 1.0f;   // main.cc:51-57
  ForkParams fork_params = ForkParams::ForReuse(0.5f);        // main.cc:191-193
  SelMultCalibration calibration;
  // false: every game starts from the empty board at `komi`, no forks (plumbing tests)
  bool init_state_sampling = true;
  float komi = 7.5f;
  bool raw_policy_opening = true;
  int cache_entries_per_game = 64;   // 0 disables the evaluation cache
  bool enable_puct_fast_search = true;
  ReuseBuffer* reuse = nullptr;      // shared by the games of one process (main.cc:186)
  GameRecorder* recorder = nullptr;  // optional
};

constexpr int kMaxNumRawPolicyMoves = 30;              // self_play_thread.cc:45
constexpr float kMoveSelectedForTrainingProb = 0.25f;  // :62
constexpr int kComputePAMoveNums[] = {200, 250, 300, 350, 400};   // :56
constexpr float kOverSearchNodeProb = 0.15f;           // :65
constexpr float kDownBadThreshold = -0.90f;            // :68
constexpr int kNumDownBadMovesThreshold = 5;           // :71
constexpr float kPuctFastSearchProb = 0.25f;           // :74

// Per-game evaluation cache: the reference keeps one LRU per game thread keyed by
// NNKey = (colour, board hash, last `num_cache_last_moves` moves, komi)
// (cc/nn/nn_interface.h:206-228, nn_interface.cc:92-118; self-play sets 1 last move,
// selfplay/main.cc:177).  Results are stored un-symmetrised, as the reference does.
class EvalCache {
 public:
  // num_last_moves: how many of the last moves are part of the key (NNInterface::
  // SetNumCacheLastMoves; self-play 1, the default used by cc/eval 5)
  explicit EvalCache(int capacity, int num_last_moves = 1) : cap_(capacity), nlast_(num_last_moves) {}
  struct Key {
    uint64_t hash;
    Loc last[5];
    float komi;
    Color color;
    bool operator==(const Key& o) const {
      if (hash != o.hash || komi != o.komi || color != o.color) return false;
      for (int i = 0; i < 5; ++i)
        if (last[i] != o.last[i]) return false;
      return true;
    }
  };
  // 128-bit digest of a key for the engine's HBM table (two independent mixes of the same fields)
  static void Digest(const Key& k, uint64_t* lo, uint64_t* hi) {
    uint32_t kb;
    std::memcpy(&kb, &k.komi, 4);
    uint64_t a = k.hash ^ (uint64_t(uint8_t(k.color)) * 0x9e3779b97f4a7c15ull);
    uint64_t b = (k.hash * 0xd6e8feb86659fd93ull) ^ (uint64_t(kb) << 8) ^ uint64_t(uint8_t(k.color));
    for (const Loc& l : k.last) {
      const uint64_t m = uint64_t(uint32_t(l.i * 32 + l.j + 64));
      a = (a ^ m) * 0xff51afd7ed558ccdull;
      b = ((b << 7) | (b >> 57)) ^ (m * 0xc2b2ae3d27d4eb4full);
    }
    a = (a ^ kb) * 0xc4ceb9fe1a85ec53ull;
    b = (b ^ (b >> 31)) * 0x94d049bb133111ebull;
    *lo = a ^ (a >> 29);
    *hi = b ^ (b >> 32);
    if ((*lo | *hi) == 0) *lo = 1;
  }
  Key MakeKey(const Position& pos, Color c) const {   // NNInterface::MakeKey, nn_interface.cc:92-106
    Key k{pos.board.hash(), {kNoopLoc, kNoopLoc, kNoopLoc, kNoopLoc, kNoopLoc}, pos.komi(), c};
    for (int i = 5 - nlast_; i < 5; ++i) k.last[i] = pos.last[i].loc;
    return k;
  }
  const p3hip_result* Find(const Key& k) {
    for (auto& e : entries_)
      if (e.key == k) { e.stamp = ++clock_; return &e.result; }
    return nullptr;
  }
  void Insert(const Key& k, const p3hip_result& r) {
    if (Entry* e = Victim()) { e->key = k; e->stamp = ++clock_; e->id = 0; e->pending = false; e->result = r; }
  }
  // Several evaluations of one game in flight (round 4): a request that misses takes its entry AT ONCE
  // (InsertPending) and the result is written into it when it arrives (Fill), so every later lookup sees the cache
  // exactly as the one-at-a-time order Find -> evaluate -> Insert -> Find ... leaves it — the same stamps, the
  // same entry evicted.  A lookup that finds a reserved entry (kPending) waits for that evaluation; an entry
  // evicted before its result arrived is simply not filled (the one-at-a-time order would have filled it and
  // then evicted it).
  enum class Lookup { kMiss, kHit, kPending };
  Lookup Probe(const Key& k, const p3hip_result** hit, uint64_t* pending_id) {
    for (auto& e : entries_)
      if (e.key == k) {
        e.stamp = ++clock_;
        if (e.pending) { *pending_id = e.id; return Lookup::kPending; }
        *hit = &e.result;
        return Lookup::kHit;
      }
    return Lookup::kMiss;
  }
  uint64_t InsertPending(const Key& k) {   // 0: no cache
    Entry* e = Victim();
    if (!e) return 0;
    e->key = k; e->stamp = ++clock_; e->id = ++next_id_; e->pending = true;
    return e->id;
  }
  void Fill(uint64_t id, const p3hip_result& r) {
    if (!id) return;
    for (auto& e : entries_)
      if (e.id == id && e.pending) { e.result = r; e.pending = false; return; }
  }
  void Clear() { entries_.clear(); }

 private:
  struct Entry { Key key; uint64_t stamp = 0, id = 0; bool pending = false; p3hip_result result; };
  Entry* Victim() {   // the entry an insertion takes: a fresh one below capacity, else the least recently used
    if (cap_ <= 0) return nullptr;
    if ((int)entries_.size() < cap_) { entries_.emplace_back(); return &entries_.back(); }
    size_t lru = 0;
    for (size_t i = 1; i < entries_.size(); ++i)
      if (entries_[i].stamp < entries_[lru].stamp) lru = i;
    return &entries_[lru];
  }
  int cap_, nlast_;
  uint64_t clock_ = 0, next_id_ = 0;
  std::vector<Entry> entries_;
};

class GameRunner {
 public:
  GameRunner(const SelfPlayConfig& cfg, uint64_t seed)
      : cfg_(cfg), prob_(seed), seed_(seed), cache_(cfg.cache_entries_per_game),
        move_sel_(kNnMctsBonus | kKldPenalty, cfg.calibration) {   // self_play_thread.cc:315-316
    NewGame();
  }

  // Advances this game until it needs a network evaluation; writes the features of the
  // position to evaluate into *f.  One evaluation in flight (the reference's order of work).
  void AdvanceToEval(p3hip_features* f) {
    if (!TryAdvance(f, 1)) {
      std::fprintf(stderr, "GameRunner::AdvanceToEval: blocked with %zu requests in flight\n", fifo_.size());
      std::abort();
    }
  }
  // Advances this game until it has a position for the engine (true: *f holds it, the request joins the
  // in-flight queue) or until nothing more can start before a result in flight arrives (false).  Up to
  // `max_inflight` playouts of one search wait for results at the same time (GumbelSearch::IssueNext); the
  // game's moves, its random draws, its cache and every result are those of max_inflight = 1.
  bool TryAdvance(p3hip_features* f, int max_inflight) {
    for (;;) {
      if (forking_) {   // the fork manager's candidate evaluations ride in the same batches, one at a time
        if (!fifo_.empty()) return false;
        Color c;
        if (!fork_->NextEval(&side_pos_, &c)) {
          forking_ = false;
          PlayMove();
          continue;
        }
        if (RequestEval(side_pos_, c, f, true)) return true;
        continue;
      }
      const GumbelSearch::Issue s = search_.IssueNext(max_inflight);
      if (s == GumbelSearch::Issue::kNeedEval) {
        if (RequestEval(*search_.eval_game(), search_.eval_color(), f, false)) return true;
        continue;
      }
      if (s == GumbelSearch::Issue::kBlocked) return false;
      FinishMove();
    }
  }
  // the engine's result for the OLDEST request that went to the engine (requests complete in order)
  void DeliverResult(p3hip_result& r) {
    if (fifo_.empty() || fifo_.front().alias_of) {   // a result nobody asked for: a scheduling bug, not something to search on
      std::fprintf(stderr, "GameRunner::DeliverResult: no engine request at the head of the queue (%zu in flight)\n", fifo_.size());
      std::abort();
    }
    Request e = std::move(fifo_.front());
    fifo_.pop_front();
    if (!cfg_.device_symmetry) UnapplySymmetry(e.sym, &r);   // nn_interface.h:263-288
    cache_.Fill(e.cache_id, r);   // nn_interface.cc:130 (the entry was reserved when the request missed)
    for (Request& w : fifo_)      // requests for the same key made while this one was in flight
      if (w.alias_of == e.cache_id && w.alias_of != 0 && !w.res) w.res.reset(new p3hip_result(r));
    Complete(e, r);
    while (!fifo_.empty() && fifo_.front().res) {
      Request a = std::move(fifo_.front());
      fifo_.pop_front();
      Complete(a, *a.res);
    }
  }
  // where the scheduler put the request TryAdvance just returned, and the slot of the oldest request if it went
  // to `lane` (-1 otherwise)
  void SetBackSlot(int lane, int slot) { fifo_.back().lane = lane; fifo_.back().slot = slot; unloaded_ = false; }
  // the request TryAdvance just returned could not be loaded (the batch had gone): it waits, in the scheduler's feature
  // buffer of this game, for the next host phase; nothing else may be requested before it is loaded
  void MarkUnloaded() { unloaded_ = true; }
  // device symmetry: the mask of the request TryAdvance just returned (still the newest while it waits unloaded)
  uint32_t BackMask() const { return 1u << (int)fifo_.back().sym; }
  bool unloaded() const { return unloaded_; }
  int FrontSlot(int lane) const {
    return !fifo_.empty() && !fifo_.front().alias_of && fifo_.front().lane == lane ? fifo_.front().slot : -1;
  }
  size_t inflight() const { return fifo_.size(); }
  const GameStats& stats() const { return stats_; }
  const Game& game() const { return *game_; }
  // false while the game still samples its opening from the raw policy (one evaluation per move,
  // self_play_thread.cc:44,363-366): the scheduler's advance phase plays every game past it
  bool past_opening() const { return game_->num_moves() >= num_moves_raw_policy_; }
  const std::vector<Move>& last_moves() const { return last_moves_; }
  uint64_t first_game_digest() const { return first_game_digest_; }   // 0 until the first game has finished
  const Game::Result& last_result() const { return last_result_; }

 private:
  struct Request {
    Symmetry sym = kIdentity;
    uint64_t cache_id = 0;    // the cache entry reserved for the result (0: none)
    uint64_t alias_of = 0;    // != 0: no engine request of its own, waits for the request that owns this entry
    bool side = false;        // a fork candidate's evaluation (ForkManager), not the search's
    int lane = -1, slot = -1;
    std::unique_ptr<p3hip_result> res;   // an alias's result, once its owner's has arrived
  };
  // true: *f holds a position for the engine; false: served from the cache (now, or when the evaluation of the
  // same key that is already in flight arrives)
  bool RequestEval(const Position& pos, Color c, p3hip_features* f, bool side) {
    const EvalCache::Key key = cache_.MakeKey(pos, c);
    const p3hip_result* hit = nullptr;
    uint64_t owner = 0;
    switch (cache_.Probe(key, &hit, &owner)) {   // nn_interface.cc:112-118
      case EvalCache::Lookup::kHit:
        ++stats_.cache_hits;
        if (side) fork_->Deliver(*hit);
        else search_.ResolveBack(*hit);
        return false;
      case EvalCache::Lookup::kPending: {
        ++stats_.cache_hits;
        Request w;
        w.alias_of = owner;
        w.side = side;
        fifo_.push_back(std::move(w));
        return false;
      }
      case EvalCache::Lookup::kMiss:
        break;
    }
    Request e;
    e.sym = RandomSymmetry(prob_.prng());   // nn_interface.cc:123
    FillFeatures(pos, c, cfg_.device_symmetry ? kIdentity : e.sym, f);   // (the draw is the host path's either way)
    ++stats_.evals;
    e.cache_id = cache_.InsertPending(key);
    e.side = side;
    fifo_.push_back(std::move(e));
    return true;
  }
  void Complete(const Request& e, const p3hip_result& r) {
    if (e.side) fork_->Deliver(r);
    else search_.Deliver(r);
  }

  void NewGame() {   // self_play_thread.cc:319-426
    InitState init;
    if (cfg_.init_state_sampling) {
      init = GetInitState(prob_, cfg_.reuse, cfg_.use_seen_state_prob);
    } else {
      init.board = Board(cfg_.komi, true);
    }
    force_full_search_first_move_ = init.first_move_behavior == FirstMoveBehavior::kForceFullSearch;
    const bool disable_sampling = init.first_move_behavior != FirstMoveBehavior::kSample;
    const bool is_fresh_game = init.kind == InitState::Kind::kEmpty || init.kind == InitState::Kind::kBook ||
                               init.kind == InitState::Kind::kHandicap;
    init_board_ = init.board;
    game_.reset(new Game(init.board, init.last_moves, init.move_num));
    color_ = init.color_to_move;
    pool_.Clear();
    // one bias cache per game (self_play_thread.cc:407-412): the old game's nodes are gone
    bias_cache_.reset(cfg_.bias_cache_lambda > 0.0f ? new BiasCache(cfg_.bias_cache_alpha, cfg_.bias_cache_lambda)
                                                    : nullptr);
    search_.set_bias_cache(bias_cache_.get());
    root_ = pool_.Create();
    move_infos_.clear();
    num_consecutive_down_bad_moves_ = 0;
    (void)prob_.Uniform();   // log_mcts_trees draw, kLogFullTreeProb = 0 (:353)
    const int max_raw = (int)std::round(kMaxNumRawPolicyMoves * std::pow(0.5f, init.move_num / 40.0f));
    num_moves_raw_policy_ = 0;
    if (cfg_.raw_policy_opening && !disable_sampling && max_raw > 0 && prob_.Uniform() < 1.0f)   // kOpeningExploreProb
      num_moves_raw_policy_ = RandRange(prob_.prng(), 0, max_raw);
    use_puct_fast_search_ = prob_.Uniform() < kPuctFastSearchProb && cfg_.enable_puct_fast_search;
    fast_move_noise_scaling_ = prob_.Uniform() / 1.4f;
    {
      int num_rounds = (int)std::log2((double)cfg_.default_k);
      int min_k = 1 << num_rounds;
      fast_move_gumbel_k_ = RandRange(prob_.prng(), min_k, cfg_.default_k + 1);
    }
    fast_move_root_fpu_ = prob_.Uniform() * 0.1f;   // :424
    fork_.reset();
    if (cfg_.init_state_sampling && cfg_.reuse)
      fork_.reset(new ForkManager(cfg_.fork_params, cfg_.reuse, prob_, /*started_from_forced_search=*/!is_fresh_game));
    forking_ = false;
    fifo_.clear();
    unloaded_ = false;
    cache_.Clear();
    if (game_->IsGameOver() || game_->num_moves() >= cfg_.max_moves) {
      // A restart state can already be finished (a fork whose alternative move was the second
      // pass): the reference's game loop (self_play_thread.cc:427-428) is then skipped and the
      // game is scored and recorded as it stands.
      FinishGame();
      return;
    }
    BeginSearch();
  }

  void FinishGame() {   // self_play_thread.cc:900-912
    game_->WriteResult();
    ++stats_.games;
    if (game_->result().winner == kBlack) ++stats_.black_wins;
    last_result_ = game_->result();
    last_moves_ = game_->moves();
    if (stats_.games == 1) {   // a digest of this runner's first game: schedules are compared by it (tests)
      uint64_t d = 0xcbf29ce484222325ull;
      for (const Move& m : last_moves_) d = (d ^ (uint64_t)(MoveIdx(m.loc) * 4 + (int)m.color + 2)) * 0x100000001b3ull;
      uint32_t bs, ws;
      std::memcpy(&bs, &last_result_.bscore, 4);
      std::memcpy(&ws, &last_result_.wscore, 4);
      first_game_digest_ = ((d ^ bs) * 0x100000001b3ull ^ ws) * 0x100000001b3ull | 1;
    }
    if (fork_) fork_->FinalizeGame(*game_, prob_);
    if (cfg_.recorder) cfg_.recorder->RecordGame(init_board_, *game_, std::move(move_infos_));
    NewGame();
  }

  void BeginSearch() {   // self_play_thread.cc:429-611
    const bool sampling_raw_policy = game_->num_moves() < num_moves_raw_policy_;
    const bool is_either_down_bad = num_consecutive_down_bad_moves_ >= kNumDownBadMovesThreshold;
    float down_bad_coeff = 1.0f;
    {
      const float root_v = VOutcome(root_);
      if (!(root_v > kDownBadThreshold && root_v < -kDownBadThreshold))
        down_bad_coeff = (1.0f - std::abs(root_v)) / (1.0f - std::abs(kDownBadThreshold));
    }
    // pre-search statistics (from tree reuse)
    pre_.sampling_raw_policy = sampling_raw_policy;
    const float qz_nn = root_->init_outcome_est;
    pre_.n_pre = root_->n;
    pre_.q_pre = V(root_);
    const float qz_pre = VOutcome(root_);
    pre_.var_pre = pre_.n_pre < 3 ? 0.0f : root_->v_outcome_var;
    pre_.pre_kld = 0.0f;
    if (root_->n >= 1) {
      float pi[kNumMoves];
      ComputeImprovedPolicyN(root_, 0, pi);
      pre_.pre_kld = ComputeKLD(pi, root_->move_probs);
    }
    const float q_canonical = qz_pre == 0.0f ? qz_nn : qz_pre;
    pre_.nn_mcts_diff_pre = pre_.n_pre > 0 ? std::abs(qz_nn - pre_.q_pre) : 0.0f;
    const MoveSelResult sel = move_sel_.Compute(pre_.n_pre, std::sqrt(pre_.var_pre), pre_.pre_kld, pre_.nn_mcts_diff_pre,
                                                q_canonical, cfg_.sel_mult_scale_factor);
    pre_.sel_mult_modifier = sampling_raw_policy ? 1.0f : sel.modifier;
    const float sel_mult = cfg_.sel_mult_base > 0.0f ? cfg_.sel_mult_base * pre_.sel_mult_modifier : 1.0f;
    float select_move_prob = 0.0f;
    pre_.select_move_prob_base = 0.0f;
    if (!sampling_raw_policy) {
      pre_.select_move_prob_base = is_either_down_bad ? down_bad_coeff * down_bad_coeff * kMoveSelectedForTrainingProb
                                                      : kMoveSelectedForTrainingProb;
      select_move_prob = pre_.select_move_prob_base * sel_mult;
    }
    int train_n = cfg_.selected_n, train_k = cfg_.selected_k;   // trainable_gumbel_params, :526-537
    if (is_either_down_bad) {
      train_n = (int)((1.0f - down_bad_coeff) * cfg_.default_n + down_bad_coeff * cfg_.selected_n);
      train_k = cfg_.default_k;
    }
    const bool force_first_move = force_full_search_first_move_ && game_->num_moves() == 0;
    const bool selected = force_first_move || prob_.Uniform() < select_move_prob;   // :541-542
    (void)prob_.Uniform();                                  // over-search draw (`&& false`, :543-545)
    pre_.selected = selected;
    GumbelParams p;
    p.nonroot_var_scale_prior_visits = cfg_.nonroot_var_scale_prior_visits;
    p.early_stopping_enabled = cfg_.early_stopping_enabled;   // (!is_move_over_search: over-search is dead code, :544-548)
    if (force_first_move) {
      p.n = cfg_.selected_n; p.k = cfg_.selected_k;
    } else if (sampling_raw_policy) {
      p.n = 1; p.k = 1;
    } else if (selected) {
      p.n = train_n; p.k = train_k;
    } else {
      p.n = cfg_.default_n; p.k = fast_move_gumbel_k_; p.noise_scaling = fast_move_noise_scaling_;
    }
    {   // tau schedule, self_play_thread.cc:570-582
      const int non_sample = game_->num_moves() - num_moves_raw_policy_;
      const float lambda = std::log(2.0f) / 19;
      p.tau = std::min(std::max(0.8f * std::exp(-lambda * non_sample), 0.2f), 0.8f);
    }
    if (!selected && !sampling_raw_policy && use_puct_fast_search_) {   // self_play_thread.cc:585-611
      PuctParams pp;
      pp.c_puct = 1.05f;
      pp.c_puct_visit_scaling = 0.28f;
      pp.root_fpu = fast_move_root_fpu_;
      search_.BeginPuct(game_.get(), &pool_, root_, color_, p.n, pp, p.tau, &prob_);
      return;
    }
    search_.Begin(game_.get(), &pool_, root_, color_, p, &prob_);
  }

  void FinishMove() {   // self_play_thread.cc:614-690
    const GumbelResult& res = search_.result();
    move_ = res.mcts_move;
    const float root_q_outcome = VOutcome(root_);
    // bias-cache adjustment of this root, read-only (self_play_thread.cc:638-641; the reference logs it)
    if (bias_cache_) stats_.bias_adj_abs_sum += std::abs(bias_cache_->Fetch(root_->bias));
    if (cfg_.recorder) {
      MoveSearchRecord mi;
      std::memcpy(mi.mcts_pi, res.pi_improved, sizeof mi.mcts_pi);
      mi.move_trainable = pre_.selected;
      mi.root_q_outcome = root_q_outcome;
      mi.root_score = root_->score;
      mi.kld = res.kld;
      std::memcpy(mi.mcts_value_dist, root_->v_categorical, sizeof mi.mcts_value_dist);
      MoveSearchStats& st = mi.move_stats;   // :654-669 (visit_count is never set there: stays 0)
      st.sampled_raw_policy = pre_.sampling_raw_policy;
      st.nn_q = root_->init_util_est;
      st.mcts_q = pre_.q_pre;
      st.nn_mcts_diff = pre_.nn_mcts_diff_pre;
      st.v_outcome_stddev = std::sqrt(pre_.var_pre);
      float ent = 0;
      for (int a = 0; a < kNumMoves; ++a)
        if (root_->move_probs[a] > 0.0f) ent -= root_->move_probs[a] * std::log(root_->move_probs[a]);
      st.prior_entropy = ent;
      st.nn_uncertainty = root_->v_err;
      st.kld = 0.0f;
      if (root_->n >= 1) {
        float pi[kNumMoves];
        ComputeImprovedPolicyN(root_, 0, pi);
        st.kld = ComputeKLD(pi, root_->move_probs);   // post_kld
      }
      st.pre_kld = pre_.pre_kld;
      st.sel_mult_modifier = pre_.sel_mult_modifier;
      st.sel_mult_modifier_weight = pre_.select_move_prob_base / kMoveSelectedForTrainingProb;
      st.visit_count_pre = (float)pre_.n_pre;
      move_infos_.push_back(mi);
    }
    if (-std::abs(root_q_outcome) < kDownBadThreshold) ++num_consecutive_down_bad_moves_;
    else num_consecutive_down_bad_moves_ = 0;
    if (fork_) {   // fork before playing the move (:681-688)
      ForkManager::MoveData md{&game_->board(), color_, move_, root_->init_util_est, V(root_), root_->score,
                               root_->child_visits(MoveIdx(move_)) != 0};
      if (fork_->MaybeFork(*game_, md, prob_)) {
        forking_ = true;
        return;
      }
    }
    PlayMove();
  }

  void PlayMove() {   // self_play_thread.cc:690-722, 900-912
    const Loc move = move_;
    game_->PlayMove(move, color_);
    ++stats_.moves;
    for (int m : kComputePAMoveNums)
      if (game_->num_moves() == m) game_->mutable_board().CalculatePassAliveRegions();
    color_ = Opp(color_);
    TreeNode* next = root_->child(MoveIdx(move));
    if (!next) next = pool_.Create();
    pool_.Reap(next);   // self_play_thread.cc:711-722
    root_ = next;
    if (bias_cache_) stats_.bias_entries_pruned += bias_cache_->PruneUnused();   // :730-733
    if (game_->IsGameOver() || game_->num_moves() >= cfg_.max_moves) {
      FinishGame();
      return;
    }
    if (root_->is_terminal) {   // cannot happen while the game is not over; defensive reset
      root_ = pool_.Create();
      pool_.Reap(root_);
    }
    BeginSearch();
  }

  struct PreSearch {
    bool sampling_raw_policy = false, selected = false;
    int n_pre = 0;
    float q_pre = 0, var_pre = 0, pre_kld = 0, nn_mcts_diff_pre = 0, sel_mult_modifier = 1, select_move_prob_base = 0;
  };

  SelfPlayConfig cfg_;
  Probability prob_;
  uint64_t seed_;
  std::unique_ptr<Game> game_;
  Board init_board_;
  std::unique_ptr<BiasCache> bias_cache_;   // declared before the pool: nodes release their entries first
  NodePool pool_;
  TreeNode* root_ = nullptr;
  Color color_ = kBlack;
  Loc move_ = kNoopLoc;
  GumbelSearch search_;
  int num_moves_raw_policy_ = 0, fast_move_gumbel_k_ = 4, num_consecutive_down_bad_moves_ = 0;
  float fast_move_noise_scaling_ = 1.0f, fast_move_root_fpu_ = 0.0f;
  bool use_puct_fast_search_ = false, force_full_search_first_move_ = false;
  bool forking_ = false;
  std::deque<Request> fifo_;   // evaluation requests in flight, oldest first
  bool unloaded_ = false;
  std::unique_ptr<ForkManager> fork_;
  Position side_pos_;
  PreSearch pre_;
  std::vector<MoveSearchRecord> move_infos_;
  EvalCache cache_;
  MoveSelManager move_sel_;
  GameStats stats_;
  Game::Result last_result_;
  std::vector<Move> last_moves_;
  uint64_t first_game_digest_ = 0;
};

}  // namespace p3
