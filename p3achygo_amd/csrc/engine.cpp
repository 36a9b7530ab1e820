// engine.cpp — the p3hip C ABI (include/p3hip.h): weight loading / repacking, pinned
// staging, slot compaction, launch sequence.  Compiled with hipcc into libp3hip.so.
//
// Replaces TrtEngineImpl (cc/nn/engine/trt_engine.cc:85-351) behind nn::Engine
// (cc/nn/engine/engine.h:22-43).  Differences by design:
//   * the GoFeatures POD itself (1,860 B) is what crosses PCIe; planes are expanded on
//     the device (go_features.cc:10-61 restated in k_init) instead of 21,692 B of fp32;
//   * only slots loaded since the previous run are uploaded and evaluated, compacted
//     into a dense batch (the TRT engine always runs the full static batch);
//   * only the consumed outputs (7,556 B / position) come back every run; ownership and
//     raw logits stay on the device until asked for.
#include <hip/hip_runtime.h>
#include <chrono>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_set>
#include <string>
#include <vector>

#include "engine.h"
#include "block_i8.h"
#include "conv_any.h"
#include "conv_f32.h"
#include "conv_split.h"
#include "conv_wino.h"
#include "edge_split.h"
#include "lconv_i8.h"
#include "loss.h"
#include "transformer.h"
#include "transformer_f32.h"
#include "transformer_split.h"

using namespace eng;

namespace {

thread_local std::string g_create_error;

// where p3hip_run / p3hip_upload put the slots' records: the forward pass's input, or the expand's
unsigned char* upload_buffer(p3hip_engine* e) { return e->any_sym() ? e->d_sfeats : e->d_feats; }

// H2D of the `n` records gather_loaded put in the dense upload
bool upload(p3hip_engine* e, int n) {
  return e->check(hipMemcpyAsync(upload_buffer(e), e->feats_identity ? e->h_feats : e->h_feats_compact,
                                 (size_t)n * kFeatBytes, hipMemcpyHostToDevice, e->stream), "H2D features");
}

// D2H of the result records of rows 0 .. n - 1 into h_out: one contiguous copy from `res` (d_res), or strided from d_out
bool download(p3hip_engine* e, int n, const float* res) {
  const size_t rec = p3::kResultFloats * 4;
  return e->check(res ? hipMemcpyAsync(e->h_out, res, n * rec, hipMemcpyDeviceToHost, e->stream)
                      : hipMemcpy2DAsync(e->h_out, rec, e->d_out, p3::kOutStride * 4, rec, n, hipMemcpyDeviceToHost, e->stream),
                  "D2H results");
}

// Frees the NN cache's buffers and leaves it off (p3hip_destroy; a p3hip_cache_enable that failed part-way)
void free_cache(p3hip_engine::DeviceCache& c) {
  hipFree(c.d_tkeys); hipFree(c.d_tmeta); hipFree(c.d_tvals); hipFree(c.d_keys); hipFree(c.d_hit); hipFree(c.d_victim);
  hipFree(c.d_lists); hipFree(c.d_sym); hipFree(c.d_feats2);
  if (c.h_keys) hipHostFree(c.h_keys);
  if (c.h_hit) hipHostFree(c.h_hit);
  if (c.h_victim) hipHostFree(c.h_victim);
  if (c.h_lists) hipHostFree(c.h_lists);
  if (c.h_sym) hipHostFree(c.h_sym);
  delete[] c.h_slot_keys;
  c = p3hip_engine::DeviceCache{};
}

// Debug read-backs: the `n` activation elements from element `first` of `buf` on, as floats, once the stream has drained
// (the fp32 paths' buffers have the same orders: the stored values themselves)
int read_acts(p3hip_engine* e, const _Float16* buf, size_t first, size_t n, float* out) {
  hipStreamSynchronize(e->stream);
  if (is_f32(e->trunk_path()))
    return hipMemcpy(out, (const float*)buf + first, n * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
  std::vector<_Float16> h(n);
  if (hipMemcpy(h.data(), buf + first, n * 2, hipMemcpyDeviceToHost) != hipSuccess) return 2;
  for (size_t i = 0; i < n; ++i) out[i] = (float)h[i];
  return 0;
}

// ---- the device buffers of an engine: their sizes, and what a forward pass may read of them ----------------------
//
// The sizes of the buffers p3hip_create allocates, from what it fixed before (batch, rows, the weight file, the plan):
// p3hip_create allocates by these and p3hip_debug_poison fills by them, so the two cannot drift apart.
size_t act_elems(const p3hip_engine* e, size_t channels) { return (size_t)e->rows * channels * kNLoc; }
size_t x_bytes(const p3hip_engine* e) { return act_elems(e, e->wf.C) * act_bytes(e->trunk_path()); }
// t holds a C-channel tensor (broadcast blocks, classic blocks, the transformer's o) or, in a layer-wise btl / nbt block,
// two C_b-channel ones side by side (enqueue_forward, regions 1 and 2): 2 C_b > C where C_b > C / 2 (P3HIP_CONV_SET
// allows C_b up to C, and padding C_b to a multiple of 64 can pass C / 2 as well)
size_t t_bytes(const p3hip_engine* e) {
  const size_t C = e->wf.C;
  const size_t Ct = (e->wf.btype == 0 || e->wf.btype == 1) ? std::max<size_t>(C, 2 * (size_t)e->wf.Cb) : C;
  return act_elems(e, Ct) * act_bytes(e->trunk_path());
}
size_t s_bytes(const p3hip_engine* e) { return act_elems(e, e->wf.Cb) * 2; }
size_t qkv_bytes(const p3hip_engine* e) {   // heads x head width = model width
  return 3 * (size_t)e->rows * p3::kTfmLPad * (size_t)e->wf.model_C * act_bytes(e->trunk_path());
}
size_t hp_bytes(const p3hip_engine* e) { return (size_t)e->rows * 96 * kNLoc * 4; }
size_t pool_bytes(const p3hip_engine* e) { return (size_t)e->rows * p3::kHeadsPoolFloats * 4; }
size_t out_bytes(const p3hip_engine* e) { return (size_t)e->batch * p3::kOutStride * 4; }
size_t cout_bytes(const p3hip_engine* e) { return (size_t)e->rows * p3::kOutStride * 4; }
size_t res_bytes(const p3hip_engine* e) { return (size_t)e->batch * p3::kResultFloats * 4; }
size_t aux_bytes(const p3hip_engine* e) { return (size_t)e->rows * p3::kAuxStride * 4; }
size_t feats_bytes(const p3hip_engine* e) { return (size_t)e->rows * kFeatBytes; }
size_t slot_feats_bytes(const p3hip_engine* e) { return (size_t)e->batch * kFeatBytes; }
size_t symtab_bytes(const p3hip_engine* e) { return (size_t)e->batch * 5; }
size_t quant_bytes(const p3hip_engine* e) { return (size_t)e->plan.n_q * 4; }
size_t arena_bytes(const p3hip_engine* e) { return e->arena_bytes; }
// (the buffers other entry points make: p3hip_cache_enable, scoring.cpp ensure_scoring, loss_abi.cpp ensure_loss, and the
// diagnostics of forward.cpp)
size_t cache_entries(const p3hip_engine* e) { return (size_t)e->cache.mask + 1; }
size_t batch_words(const p3hip_engine* e) { return (size_t)e->batch * 4; }

// q, k, v are [3][rows][head][384][D]: token rows 0 .. 360 of every head are what a block writes and reads; rows
// 361 .. 383 are zeroed by p3hip_create and never written (transformer.h kTfmLPad), and the attention kernels read them
// as keys and values.  Fills the 361 written rows of every head and leaves the 23 others alone.
bool poison_qkv_tokens(p3hip_engine* e, int byte) {
  const size_t eb = act_bytes(e->trunk_path()), D = (size_t)e->plan.choice.tfm_D;
  const size_t heads = (size_t)e->plan.choice.tfm_heads;
  return e->check(hipMemset2DAsync(e->d_qkv, p3::kTfmLPad * D * eb, byte, (size_t)kNLoc * D * eb, 3 * (size_t)e->rows * heads, e->stream),
                  "poison q, k, v");
}

// What a forward pass may read of a device buffer ("What a forward pass may read"):
//   Poisoned    values that a pass, or the entry point that reads them, must write before it reads them: whatever they
//               held before must not reach an output.  p3hip_debug_poison fills them.
//   State       what outlives a pass by design: weights, calibration, the cache's table, labels and targets, diagnostics.
//   Index       records the kernels or the host compute addresses from (features, symmetry tables, the cache's keys and
//               lists, the rows of scoring and loss).  Never filled: no run may address through poison.
//   ZeroedOnce  zeroed by p3hip_create and never written in part (zero_range); the rest is filled as Poisoned.
enum class BufClass { Poisoned, State, Index, ZeroedOnce };

const char* class_name(BufClass c) {
  switch (c) {
    case BufClass::Poisoned: return "poisoned";
    case BufClass::State: return "state";
    case BufClass::Index: return "index";
    case BufClass::ZeroedOnce: return "zeroed-once";
  }
  return "";
}

struct DeviceBuffer {
  const char* name;                         // the member of p3hip_engine, as engine.h spells it (nested: struct.member)
  void* (*ptr)(const p3hip_engine*);        // null: this engine has no such buffer
  size_t (*bytes)(const p3hip_engine*);
  BufClass cls;
  const char* zero_range = "";                            // ZeroedOnce: the part that stays zero, in words
  bool (*poison_rest)(p3hip_engine*, int) = nullptr;      // ZeroedOnce: fills everything outside zero_range
};

#define P3_BUF(member) #member, [](const p3hip_engine* e) -> void* { return (void*)e->member; }
#define P3_BYTES(expr) [](const p3hip_engine* e) -> size_t { return expr; }

// Every device pointer member of p3hip_engine, once (tests/test_scratch_poison_cpu.py holds engine.h against this table).
const DeviceBuffer kDeviceBuffers[] = {
    // the forward pass's activations and head scratch: every pass writes what it reads of them
    {P3_BUF(d_x), x_bytes, BufClass::Poisoned},
    {P3_BUF(d_t), t_bytes, BufClass::Poisoned},
    {P3_BUF(d_u), x_bytes, BufClass::Poisoned},
    {P3_BUF(d_s), s_bytes, BufClass::Poisoned},
    {P3_BUF(d_qkv), qkv_bytes, BufClass::ZeroedOnce, "token rows 361..383 of every head of q, k and v", poison_qkv_tokens},
    {P3_BUF(d_hp), hp_bytes, BufClass::Poisoned},
    {P3_BUF(d_pool), pool_bytes, BufClass::Poisoned},
    // the output rows: a run writes the rows it hands out
    {P3_BUF(d_cout), cout_bytes, BufClass::Poisoned},
    {P3_BUF(d_out), out_bytes, BufClass::Poisoned},
    {P3_BUF(d_res), res_bytes, BufClass::Poisoned},
    {P3_BUF(d_aux), aux_bytes, BufClass::Poisoned},
    // p3hip_score and p3hip_loss write the terms and sums they copy back
    {P3_BUF(scoring.d_terms), P3_BYTES(batch_words(e) * P3HIP_NUM_SCORE_TERMS), BufClass::Poisoned},
    {P3_BUF(scoring.d_sums), P3_BYTES(P3HIP_NUM_SCORE_TERMS * sizeof(double)), BufClass::Poisoned},
    {P3_BUF(loss.d_terms), P3_BYTES(batch_words(e) * P3HIP_NUM_LOSS_TERMS), BufClass::Poisoned},
    {P3_BUF(loss.d_sums), P3_BYTES(P3HIP_NUM_LOSS_TERMS * sizeof(double)), BufClass::Poisoned},
    // state
    {P3_BUF(d_arena), arena_bytes, BufClass::State},
    {P3_BUF(d_amax), quant_bytes, BufClass::State},
    {P3_BUF(d_ascale), quant_bytes, BufClass::State},
    {P3_BUF(cache.d_tkeys), P3_BYTES(cache_entries(e) * 16), BufClass::State},
    {P3_BUF(cache.d_tmeta), P3_BYTES(cache_entries(e) * 4), BufClass::State},
    {P3_BUF(cache.d_tvals), P3_BYTES(cache_entries(e) * p3::kOutStride * 4), BufClass::State},
    {P3_BUF(scoring.d_labels), P3_BYTES((size_t)e->batch * sizeof(p3hip_labels)), BufClass::State},
    {P3_BUF(loss.d_targets), P3_BYTES(batch_words(e) * p3::kTgtStride), BufClass::State},
    {P3_BUF(d_bw_stamps), P3_BYTES((size_t)8 * 16 * 4 * 24 * 8), BufClass::State},
#ifdef P3_DIAG
    {P3_BUF(d_stamps), P3_BYTES((size_t)p3::kStampWgs * 8 * p3::kStampSections * p3::kStampSlots * 8), BufClass::State},
    {P3_BUF(d_spans), P3_BYTES((size_t)p3::kSpanWgs * p3::kSpanSlots * 8), BufClass::State},
#else
    {"d_stamps", [](const p3hip_engine*) -> void* { return nullptr; }, P3_BYTES(0), BufClass::State},
    {"d_spans", [](const p3hip_engine*) -> void* { return nullptr; }, P3_BYTES(0), BufClass::State},
#endif
    // index
    {P3_BUF(d_feats), feats_bytes, BufClass::Index},
    {P3_BUF(d_sfeats), slot_feats_bytes, BufClass::Index},
    {P3_BUF(d_symtab), symtab_bytes, BufClass::Index},
    {P3_BUF(cache.d_keys), P3_BYTES((size_t)e->batch * sizeof(p3::CacheKey)), BufClass::Index},
    {P3_BUF(cache.d_hit), batch_words, BufClass::Index},
    {P3_BUF(cache.d_victim), batch_words, BufClass::Index},
    {P3_BUF(cache.d_lists), P3_BYTES(5 * batch_words(e)), BufClass::Index},
    {P3_BUF(cache.d_sym), batch_words, BufClass::Index},
    {P3_BUF(cache.d_feats2), slot_feats_bytes, BufClass::Index},
    {P3_BUF(scoring.d_rows), batch_words, BufClass::Index},
    {P3_BUF(loss.d_rows), batch_words, BufClass::Index},
};

#undef P3_BUF
#undef P3_BYTES

}  // namespace

extern "C" {

const char* p3hip_create_error(void) { return g_create_error.c_str(); }
int p3hip_graph_state(const p3hip_engine* e) {
  return e->graph_failed ? -1 : (e->graph_exec || e->graph_table.held() > 0 ? 1 : 0);
}

int p3hip_graph_stats(const p3hip_engine* e, uint64_t out[5]) {
  for (int i = 0; i < 5; ++i) out[i] = 0;
  if (!(e->flags & (P3HIP_FLAG_LAUNCH_GRAPH | P3HIP_FLAG_LAUNCH_GRAPH_ANY))) return 1;
  if (e->graph_any()) {
    const gt::Table& t = e->graph_table;
    out[0] = (uint64_t)t.held(); out[1] = t.captures(); out[2] = t.replays(); out[3] = t.launches(); out[4] = t.evictions();
  } else {
    out[0] = e->graph_exec ? 1 : 0; out[1] = e->graph_captures; out[2] = e->graph_replays; out[3] = e->graph_launched;
  }
  return 0;
}

int p3hip_debug_graph_table(const int* npos, const int* total, int n, int capacity, int* action, int* evicted) {
  if (!npos || !total || !action || !evicted || n < 0 || capacity < gt::kMinCapacity || capacity > gt::kMaxCapacity) return 1;
  gt::Table table(capacity);
  static const char feats = 0, res = 0;   // the buffer and the target of every key: any two fixed addresses
  for (int i = 0; i < n; ++i) {
    const gt::Step s = table.see(gt::Key{npos[i], total[i], &feats, &res}, i);
    action[i] = (int)s.action;
    evicted[i] = (int)s.evicted_tag;
  }
  return 0;
}

p3hip_engine* p3hip_create(const char* weights_path, int batch_size, int version,
                           int device_ordinal, uint32_t flags) {
  return p3hip_create_rows(weights_path, batch_size, version, device_ordinal, flags, 0);
}

p3hip_engine* p3hip_create_rows(const char* weights_path, int batch_size, int version,
                                int device_ordinal, uint32_t flags, int symmetry_rows) {
  g_create_error.clear();
  if (version != 1) { g_create_error = "only model version 1 (15 planes + 8 scalars) is supported"; return nullptr; }
  if (batch_size < 1 || batch_size > (1 << 16)) { g_create_error = "bad batch size"; return nullptr; }
  const bool sym = (flags & P3HIP_FLAG_SYMMETRY_AVG) != 0;
  const bool sym_slot = (flags & P3HIP_FLAG_SYMMETRY_SLOT) != 0;
  if (sym_slot && sym) {
    g_create_error = "P3HIP_FLAG_SYMMETRY_SLOT cannot be combined with P3HIP_FLAG_SYMMETRY_AVG: a slot's symmetries come "
                     "either from the engine's mask or from its own";
    return nullptr;
  }
  if (sym_slot && (flags & P3HIP_FLAG_AUX)) {
    g_create_error = "P3HIP_FLAG_AUX cannot be combined with P3HIP_FLAG_SYMMETRY_SLOT: the aux record holds tanh, absolute "
                     "value and softmax outputs, and their average over symmetries is nothing the reference defines";
    return nullptr;
  }
  if (!sym_slot && symmetry_rows != 0) {
    g_create_error = "symmetry_rows " + std::to_string(symmetry_rows) + " given without P3HIP_FLAG_SYMMETRY_SLOT: only such "
                     "an engine has a row capacity of its own";
    return nullptr;
  }
  if (sym_slot) {
    const long full = (long)p3::kNumSyms * batch_size;
    const long want = symmetry_rows == 0 ? full : (long)symmetry_rows;   // 0: every slot under all eight
    if (want < batch_size || want > full) {
      g_create_error = "P3HIP_FLAG_SYMMETRY_SLOT: symmetry_rows " + std::to_string(want) + " is outside batch size " +
                       std::to_string(batch_size) + " .. 8 x batch size " + std::to_string(full);
      return nullptr;
    }
    if (want > (1 << 16)) {
      g_create_error = "P3HIP_FLAG_SYMMETRY_SLOT: symmetry_rows " + std::to_string(want) +
                       " exceeds the engine's row limit of 65536 (symmetry_rows 0 means 8 x batch size)";
      return nullptr;
    }
    symmetry_rows = (int)want;
  }
  if (sym && (size_t)p3::kNumSyms * batch_size > (1u << 16)) {
    g_create_error = "P3HIP_FLAG_SYMMETRY_AVG evaluates 8 copies of every slot: 8 x batch size " +
                     std::to_string(batch_size) + " exceeds the engine's row limit of 65536 (batch size at most 8192)";
    return nullptr;
  }
  if (sym && (flags & P3HIP_FLAG_AUX)) {
    g_create_error = "P3HIP_FLAG_AUX cannot be combined with P3HIP_FLAG_SYMMETRY_AVG: the aux record holds tanh, absolute "
                     "value and softmax outputs, and their average over symmetries is nothing the reference defines";
    return nullptr;
  }
  p3hip_engine* e = new p3hip_engine();
  e->path = weights_path;
  e->batch = batch_size;
  e->device = device_ordinal;
  e->flags = flags;
  e->opt = Options::from_env();
  if (e->graph_any()) {   // (a P3HIP_GRAPH_CACHE outside 1..1024: build_plan refuses below)
    e->graph_table = gt::Table(e->opt.graph_cache, e->opt.graph_min_seen);
    e->graph_slots.resize((size_t)e->opt.graph_cache);
  }
  e->sym = sym;
  e->sym_slot = sym_slot;
  e->rows = sym ? p3::kNumSyms * batch_size : sym_slot ? symmetry_rows : batch_size;
  auto fail = [&](const std::string& m) {
    g_create_error = m;
    p3hip_destroy(e);
    return (p3hip_engine*)nullptr;
  };
  if (!e->wf.load(weights_path, e->err)) return fail(e->err);
  // host-side plan first (weight repacking; no HIP call): a bad file fails here, GPU or not
  Arena ar;
  if (!build_plan(e->wf, flags, e->opt, e->plan, ar, e->err)) return fail(e->err);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_ordinal)
    return fail("no HIP device " + std::to_string(device_ordinal) + " (the HIP engine has no CPU fallback)");
  if (!e->check(hipSetDevice(device_ordinal), "hipSetDevice")) return fail(e->err);
  hipDeviceProp_t prop;
  if (!e->check(hipGetDeviceProperties(&prop, device_ordinal), "hipGetDeviceProperties")) return fail(e->err);
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(std::string("device is ") + prop.gcnArchName + ", this engine is built for gfx950 only");
  e->n_cu = prop.multiProcessorCount;
  const size_t B = batch_size;
  // the per-row device buffers have e->rows rows: 8 x batch copies with P3HIP_FLAG_SYMMETRY_AVG, symmetry_rows with
  // P3HIP_FLAG_SYMMETRY_SLOT.  Their sizes: the functions in front of kDeviceBuffers
  const bool copies = sym || sym_slot;
  const Path path = e->trunk_path();
  e->arena_bytes = ar.host.size();
  bool ok = e->check(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking), "hipStreamCreate") &&
            e->check(hipMalloc((void**)&e->d_arena, arena_bytes(e)), "hipMalloc arena") &&
            // on the engine's own stream: it is non-blocking (no implicit ordering with the null stream a plain
            // hipMemcpy / hipMemset runs on), and the first run must find the weights there
            e->check(hipMemcpyAsync(e->d_arena, ar.host.data(), ar.host.size(), hipMemcpyHostToDevice, e->stream), "upload weights") &&
            e->check(hipHostMalloc((void**)&e->h_feats, B * kFeatBytes, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&e->h_feats_compact, B * kFeatBytes, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&e->h_out, B * p3::kResultFloats * 4, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipMalloc((void**)&e->d_res, res_bytes(e)), "hipMalloc results") &&
            e->check(hipMalloc((void**)&e->d_feats, feats_bytes(e)), "hipMalloc feats") &&
            e->check(hipMalloc((void**)&e->d_x, x_bytes(e)), "hipMalloc x") &&
            e->check(hipMalloc((void**)&e->d_t, t_bytes(e)), "hipMalloc t") &&
            e->check(hipMalloc((void**)&e->d_u, x_bytes(e)), "hipMalloc u") &&
            // (d_s is the fused nbt kernel's scratch; the fp32 plan runs layer by layer and has none)
            (e->wf.btype != 1 || path == Path::F32Conv || e->check(hipMalloc((void**)&e->d_s, s_bytes(e)), "hipMalloc s")) &&
            (!is_tfm(path) || e->check(hipMalloc((void**)&e->d_qkv, qkv_bytes(e)), "hipMalloc qkv")) &&
            e->check(hipMalloc((void**)&e->d_hp, hp_bytes(e)), "hipMalloc hp") &&
            // (the split heads' pooled values, edge_split.h: the two low-latency paths only)
            ((path != Path::Split && path != Path::TfmSplit) ||
             e->check(hipMalloc((void**)&e->d_pool, pool_bytes(e)), "hipMalloc pooled")) &&
            e->check(hipMalloc((void**)&e->d_out, out_bytes(e)), "hipMalloc out") &&
            (!copies || (e->check(hipMalloc((void**)&e->d_sfeats, slot_feats_bytes(e)), "hipMalloc symmetry upload") &&
                         e->check(hipMalloc((void**)&e->d_cout, cout_bytes(e)), "hipMalloc copy rows"))) &&
            (!sym_slot || (e->check(hipMalloc((void**)&e->d_symtab, symtab_bytes(e)), "hipMalloc symmetry table") &&
                           e->check(hipHostMalloc((void**)&e->h_symtab, B * 5, hipHostMallocDefault), "hipHostMalloc") &&
                           e->check(hipMemsetAsync(e->d_symtab, 0, symtab_bytes(e), e->stream), "hipMemset symmetry table"))) &&
            (!(flags & P3HIP_FLAG_AUX) || (e->check(hipMalloc((void**)&e->d_aux, aux_bytes(e)), "hipMalloc aux") &&
                                           e->check(hipMemsetAsync(e->d_aux, 0, aux_bytes(e), e->stream), "hipMemset aux"))) &&
            (!is_int8(path) || (e->check(hipMalloc((void**)&e->d_amax, quant_bytes(e)), "hipMalloc amax") &&
                          e->check(hipMalloc((void**)&e->d_ascale, quant_bytes(e)), "hipMalloc scales") &&
                          e->check(hipMemsetAsync(e->d_amax, 0, quant_bytes(e), e->stream), "hipMemset amax") &&
                          e->check(hipMemsetAsync(e->d_ascale, 0, quant_bytes(e), e->stream), "hipMemset scales")));
  if (!ok) return fail(e->err);
  e->h_scale.assign(e->plan.n_q, 0.0f);
  memset(e->h_feats, 0, B * kFeatBytes);
  if (!e->check(hipMemsetAsync(e->d_feats, 0, feats_bytes(e), e->stream), "hipMemset feats") ||
      (copies && !e->check(hipMemsetAsync(e->d_sfeats, 0, slot_feats_bytes(e), e->stream), "hipMemset symmetry upload")) ||
      (copies && !e->check(hipMemsetAsync(e->d_cout, 0, cout_bytes(e), e->stream), "hipMemset copy rows")) ||
      (is_tfm(path) && !e->check(hipMemsetAsync(e->d_qkv, 0, qkv_bytes(e), e->stream), "hipMemset qkv")) ||
      !e->check(hipMemsetAsync(e->d_out, 0, out_bytes(e), e->stream), "hipMemset out") ||
      !e->check(hipStreamSynchronize(e->stream), "upload sync")) return fail(e->err);
  // the heads' arguments that never change: the weight pointers, by the table that packed them
  e->heads_args.conv_a = e->d_arena + e->plan.heads_conv_a_off;
  e->heads_args.image = e->dev<float>(e->plan.heads_image_off);
  e->heads_args.V = e->wf.V;
  e->heads_args.gbn_scale = e->dev<float>(e->plan.heads_gbn.scale_off);
  e->heads_args.gbn_shift = e->dev<float>(e->plan.heads_gbn.shift_off);
  for (int k = 0; k < kNumHeadTensors; ++k) e->heads_args.*kHeadTensors[k].arg = e->dev<float>(e->plan.head_tensor_off[k]);
  if (flags & P3HIP_FLAG_AUX) {
    e->aux_args.V = e->wf.V;
    e->aux_args.gbn_scale = e->heads_args.gbn_scale; e->aux_args.gbn_shift = e->heads_args.gbn_shift;
    e->aux_args.gd_w = e->heads_args.gd_w; e->aux_args.gd_b = e->heads_args.gd_b;
    e->aux_args.oq_embed_w = e->heads_args.oq_embed_w; e->aux_args.oq_embed_b = e->heads_args.oq_embed_b;
    for (int k = 0; k < kNumAuxTensors; ++k) e->aux_args.*kAuxTensors[k].arg = e->dev<float>(e->plan.aux_tensor_off[k]);
  }
  e->slots = p3::SlotStates((int)B);
  e->slot_sym.assign(B, 0);
  e->row_sym.assign(B, 0);
  e->slot_mask.assign(B, 1);
  e->row_mask.assign(B, 1);
  e->has_labels.assign(B, 0);
  e->has_targets.assign(B, 0);
  e->load_seq.assign(B, 0);
  e->run_load_seq.assign(B, 0);
  return e;
}

void p3hip_destroy(p3hip_engine* e) {
  if (!e) return;
  if (e->stream || e->d_arena) (void)hipSetDevice(e->device);
  if (e->stream) hipStreamSynchronize(e->stream);
  hipFree(e->d_arena); hipFree(e->d_feats); hipFree(e->d_x); hipFree(e->d_t); hipFree(e->d_u); hipFree(e->d_s);
  hipFree(e->d_hp); hipFree(e->d_pool); hipFree(e->d_out); hipFree(e->d_res); hipFree(e->d_qkv);
  hipFree(e->d_sfeats); hipFree(e->d_cout); hipFree(e->d_aux); hipFree(e->d_symtab);
  if (e->h_symtab) hipHostFree(e->h_symtab);
  hipFree(e->d_bw_stamps);
  hipFree(e->d_amax); hipFree(e->d_ascale);
  if (e->bw_mod) hipModuleUnload(e->bw_mod);
  free_cache(e->cache);
  free_scoring(e);
  free_loss(e);
  if (e->h_feats) hipHostFree(e->h_feats);
  if (e->h_feats_compact) hipHostFree(e->h_feats_compact);
  if (e->h_out) hipHostFree(e->h_out);
  for (hipEvent_t ev : e->blk_ev) hipEventDestroy(ev);
  drop_graph(e);
  if (e->stream) hipStreamDestroy(e->stream);
  delete e;
}

const char* p3hip_debug_plan(const char* weights_path, uint32_t flags, int* n_q, uint64_t* digest) {
  g_create_error.clear();
  WeightFile wf;
  Plan plan;
  Arena ar;
  std::string err;
  if (!wf.load(weights_path, err) || !build_plan(wf, flags, Options::from_env(), plan, ar, err)) {
    g_create_error = err;
    return nullptr;
  }
  uint64_t h = 0;
  bool any_q = false;
  auto fold = [&](size_t off, size_t bytes) {
    for (size_t i = 0; i < bytes; ++i) h = (h ^ ar.host[off + i]) * 1099511628211ull;
  };
  for (const BlockPlan& b : plan.blocks)
    for (const LayerPlan& lp : b.layers)
      if (lp.qidx >= 0) {
        if (!any_q) h = 14695981039346656037ull;
        any_q = true;
        fold(lp.q_off, (size_t)lp.kw * lp.kw * lp.cin * lp.cout);
        fold(lp.qs_off, (size_t)lp.cout * 4);
      }
  if (n_q) *n_q = plan.n_q;
  if (digest) *digest = h;
  return path_name(plan.choice.path);
}

int p3hip_debug_split(int npos, int kw, int cout, int n_cu, int* strips, int* tile) {
  const Options opt = Options::from_env();
  if (npos < 1 || (kw != 1 && kw != 3) || cout < 64 || cout % 64 != 0 || n_cu < 1 || !strips || !tile || opt.split_bad) return 1;
  if (opt.split_s) { *strips = opt.split_s; *tile = opt.split_t; }
  else p3::sconv_split(npos, kw, cout, n_cu, strips, tile);
  return 0;
}

int p3hip_debug_edge_split(int npos, int c_pad, int n_cu, int* stem, int* dense, int* heads) {
  if (stem) *stem = 1;
  if (dense) *dense = 1;
  if (heads) *heads = 1;
  const Options opt = Options::from_env();
  if (npos < 1 || !p3::edge_width_ok(c_pad) || n_cu < 1 || !stem || !dense || !heads || opt.edge_bad) return 1;
  if (opt.edge_s) {
    if (!p3::edge_split_valid(c_pad, opt.edge_s, opt.edge_d, opt.edge_h)) return 1;
    *stem = opt.edge_s; *dense = opt.edge_d; *heads = opt.edge_h;
  } else {
    p3::edge_split(npos, c_pad, n_cu, stem, dense, heads);
  }
  return 0;
}

int p3hip_debug_tfm_split(int npos, int heads, int n_cu, int* parts, int* tokens) {
  const Options opt = Options::from_env();
  if (npos < 1 || heads < 1 || n_cu < 1 || !parts || !tokens || opt.tfm_split_bad) return 1;
  if (opt.tfm_split_s) { *parts = opt.tfm_split_s; *tokens = opt.tfm_split_t; }
  else p3::tfm_split(npos, heads, n_cu, parts, tokens);
  return 0;
}

long p3hip_debug_pack_sconv(const float* w, int taps, int cin, int cout, int cin_pad, int cout_pad, uint16_t* out, long n) {
  std::vector<_Float16> img;
  p3::pack_sconv(img, w, taps, cin, cout, cin_pad, cout_pad);
  for (long i = 0; i < n && i < (long)img.size(); ++i) memcpy(out + i, &img[i], 2);
  return (long)img.size();
}

long p3hip_debug_pack_wconv(const float* w, int cin, int cout, int cin_pad, int cout_pad, uint16_t* out, long n) {
  std::vector<_Float16> img;
  p3::pack_wconv(img, w, cin, cout, cin_pad, cout_pad);
  for (long i = 0; i < n && i < (long)img.size(); ++i) memcpy(out + i, &img[i], 2);
  return (long)img.size();
}

int p3hip_debug_wconv_grid(int npos, int cout, int n_cu, int* grid, long* units, long unit, long* tile0, int* ntiles, int* cout0) {
  if (npos < 1 || cout < 64 || cout > p3::kWinoMaxC || cout % 64 != 0 || n_cu < 1 || !grid || !units) return 1;
  *grid = p3::wconv_grid(npos, cout, n_cu);
  *units = p3::wconv_units(npos, cout);
  if (unit < 0 || unit >= *units) return (tile0 || ntiles || cout0) ? 1 : 0;
  long t0 = 0;
  int nt = 0, c0 = 0;
  p3::wconv_unit(npos, cout, unit, &t0, &nt, &c0);
  if (tile0) *tile0 = t0;
  if (ntiles) *ntiles = nt;
  if (cout0) *cout0 = c0;
  return 0;
}

int p3hip_kind(const p3hip_engine*) { return P3HIP_KIND_HIP; }
const char* p3hip_path(const p3hip_engine* e) { return e->path.c_str(); }
int p3hip_batch_size(const p3hip_engine* e) { return e->batch; }
const char* p3hip_last_error(const p3hip_engine* e) { return e->err.c_str(); }

int p3hip_load_slot(p3hip_engine* e, int slot, const p3hip_features* f) {
  if (slot < 0 || slot >= e->batch) return 1;
  memcpy(e->h_feats + (size_t)slot * kFeatBytes, f, kFeatBytes);
  e->slot_sym[slot] = 0;
  e->slot_mask[slot] = 1;
  e->has_labels[slot] = 0;   // labels and targets belong to one load (p3hip_load_labels, p3hip_load_targets)
  e->has_targets[slot] = 0;
  ++e->load_seq[slot];
  if (e->cache.on) e->cache.h_slot_keys[slot] = p3::CacheKey{0, 0, 0};   // no key: evaluated, never cached
  e->slots.loaded(slot);
  return 0;
}

int p3hip_load_slot_keyed(p3hip_engine* e, int slot, const p3hip_features* f, uint64_t key_lo, uint64_t key_hi, int symmetry) {
  if (slot < 0 || slot >= e->batch) return 1;
  if (symmetry < 0 || symmetry > 7) return 1;
  memcpy(e->h_feats + (size_t)slot * kFeatBytes, f, kFeatBytes);
  e->slot_sym[slot] = (unsigned char)symmetry;
  e->slot_mask[slot] = 1;
  e->has_labels[slot] = 0;
  e->has_targets[slot] = 0;
  ++e->load_seq[slot];
  if (e->cache.on) e->cache.h_slot_keys[slot] = p3::CacheKey{key_lo, key_hi, (unsigned long long)symmetry};
  e->slots.loaded(slot);
  return 0;
}

int p3hip_cache_enable(p3hip_engine* e, int log2_entries) {
  if (e->flags & P3HIP_FLAG_AUX) {
    e->err = "p3hip_cache_enable: not available on a P3HIP_FLAG_AUX engine: the table's entries are output rows of "
             "kOutStride floats with no room for the aux record, so a hit could not serve p3hip_get_aux";
    return 1;
  }
  if (!e->bind()) return 1;
  if (e->cache.on) { e->err = "cache already enabled"; return 1; }
  if (log2_entries < 4 || log2_entries > 26) { e->err = "cache size: 2^4 .. 2^26 entries"; return 1; }
  auto& c = e->cache;
  const size_t cap = (size_t)1 << log2_entries, B = (size_t)e->batch;
  bool ok = e->check(hipMalloc((void**)&c.d_tkeys, cap * 16), "hipMalloc cache keys") &&
            e->check(hipMalloc((void**)&c.d_tmeta, cap * 4), "hipMalloc cache meta") &&
            e->check(hipMalloc((void**)&c.d_tvals, cap * p3::kOutStride * 4), "hipMalloc cache records") &&
            e->check(hipMalloc((void**)&c.d_keys, B * sizeof(p3::CacheKey)), "hipMalloc") &&
            e->check(hipMalloc((void**)&c.d_hit, B * 4), "hipMalloc") && e->check(hipMalloc((void**)&c.d_victim, B * 4), "hipMalloc") &&
            e->check(hipMalloc((void**)&c.d_lists, 5 * B * 4), "hipMalloc") && e->check(hipMalloc((void**)&c.d_sym, B * 4), "hipMalloc") &&
            e->check(hipMalloc((void**)&c.d_feats2, B * kFeatBytes), "hipMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_keys, B * sizeof(p3::CacheKey), hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_hit, B * 4, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_victim, B * 4, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_lists, 5 * B * 4, hipHostMallocDefault), "hipHostMalloc") &&
            e->check(hipHostMalloc((void**)&c.h_sym, B * 4, hipHostMallocDefault), "hipHostMalloc") &&
            // (the engine's stream, as in p3hip_create: the table must be empty before the first probe kernel)
            e->check(hipMemsetAsync(c.d_tkeys, 0, cap * 16, e->stream), "hipMemset") &&
            e->check(hipMemsetAsync(c.d_tmeta, 0, cap * 4, e->stream), "hipMemset") &&
            e->check(hipStreamSynchronize(e->stream), "cache table sync");
  if (!ok) {
    // free what was allocated (an over-large table fails at the records): a later, smaller enable starts clean
    const std::string why = e->err;
    free_cache(c);
    (void)hipGetLastError();   // the failed allocation's sticky error
    e->err = why;
    return 1;
  }
  c.h_slot_keys = new p3::CacheKey[B]();
  c.out_row.assign(B, -1);
  c.was_hit.assign(B, 0);
  c.mask = (unsigned)(cap - 1);
  c.run = 0;
  c.on = true;
  return 0;
}

int p3hip_cache_stats(const p3hip_engine* e, uint64_t out[4]) {
  out[0] = e->cache.lookups; out[1] = e->cache.hits; out[2] = e->cache.inserts; out[3] = e->cache.on ? (uint64_t)e->cache.mask + 1 : 0;
  return e->cache.on ? 0 : 1;
}

// Compacts every dirty slot (loaded and not yet fetched, slot_state.h) into the dense upload.
static int gather_loaded(p3hip_engine* e) {
  const bool all = (e->flags & P3HIP_FLAG_RUN_ALL_SLOTS) != 0;
  e->gather_seq = ++e->run_seq;   // the rows change hands: the last p3hip_score's terms are no longer the slots'
  // When every slot of the static batch is evaluated (the common case: NNInterface fills the whole batch, the self-play
  // scheduler always does) the dense upload IS h_feats: no second host copy of 1.9 MB per run.
  std::vector<std::pair<int, int>> moved;
  bool identity = true;
  const int n = e->slots.gather(all, [&](int s, int row) {
    if (s != row) identity = false;
    moved.emplace_back(s, row);
    e->row_sym[row] = e->slot_sym[s];
    e->row_mask[row] = e->slot_mask[s];
    e->run_load_seq[s] = e->load_seq[s];
    if (e->cache.on) {
      e->cache.h_keys[row] = e->cache.h_slot_keys[s];
      e->cache.out_row[row] = row;   // p3hip_run re-maps (misses first, then hits)
      e->cache.was_hit[row] = 0;
      e->cache.h_sym[row] = (unsigned)e->cache.h_slot_keys[s].sym;
    }
  });
  e->feats_identity = identity && n == e->batch && !e->cache.on;
  if (!e->feats_identity)
    for (const auto& m : moved)
      memcpy(e->h_feats_compact + (size_t)m.second * kFeatBytes, e->h_feats + (size_t)m.first * kFeatBytes, kFeatBytes);
  e->last_n = n;
  return n;
}

// P3HIP_FLAG_SYMMETRY_SLOT: the table of the rows gather_loaded compacted.  When their copies exceed the engine's rows
// nothing is queued, no slot keeps a row (p3hip_get_slot answers 2) and every slot stays pending for the next run.
static bool stage_gathered(p3hip_engine* e, int n) {
  if (!e->sym_slot || stage_sym_table(e, e->row_mask.data(), n)) return true;
  e->slots.drop_rows();
  e->last_n = 0;
  return false;
}

// An INT8 engine runs only once it has activation scales (the reference refuses --use_int8 without a calibration set);
// every entry point that enqueues a forward pass checks it
static bool int8_ready(p3hip_engine* e) {
  if (!is_int8(e->trunk_path()) || e->calibrating || e->have_scales) return true;
  e->err = "INT8 engine has no activation scales: run p3hip_int8_calibrate on calibration batches or load a saved "
           "calibration with p3hip_int8_set_scales first";
  return false;
}

int p3hip_int8_calibrate(p3hip_engine* e) {
  if (!is_int8(e->trunk_path())) { e->err = "p3hip_int8_calibrate: the engine was not created with P3HIP_FLAG_INT8"; return 1; }
  if (!e->bind()) return 1;
  e->calibrating = true;
  e->last_n = 0;
  const int rc = p3hip_run(e);
  e->calibrating = false;
  if (rc != 0) return rc;
  if (e->last_n <= 0) { e->err = "p3hip_int8_calibrate: no loaded positions to calibrate on"; return 1; }
  std::vector<unsigned> bits(e->plan.n_q);
  if (!e->check(hipMemcpyAsync(bits.data(), e->d_amax, (size_t)e->plan.n_q * 4, hipMemcpyDeviceToHost, e->stream), "D2H amax") ||
      !e->check(hipStreamSynchronize(e->stream), "sync")) return 1;
  for (int i = 0; i < e->plan.n_q; ++i) {
    float m;
    memcpy(&m, &bits[i], 4);
    e->h_scale[i] = m / 127.0f;
  }
  if (!e->check(hipMemcpyAsync(e->d_ascale, e->h_scale.data(), (size_t)e->plan.n_q * 4, hipMemcpyHostToDevice, e->stream), "H2D scales") ||
      !e->check(hipStreamSynchronize(e->stream), "sync")) return 1;
  e->have_scales = true;
  return 0;
}

int p3hip_int8_scales(const p3hip_engine* e, float* out, int n) {
  if (!is_int8(e->trunk_path())) return -1;
  for (int i = 0; i < n && i < e->plan.n_q; ++i) out[i] = e->h_scale[i];
  return e->plan.n_q;
}

int p3hip_int8_set_scales(p3hip_engine* e, const float* scales, int n) {
  if (!is_int8(e->trunk_path())) { e->err = "p3hip_int8_set_scales: the engine was not created with P3HIP_FLAG_INT8"; return 1; }
  if (n != e->plan.n_q) {
    e->err = "p3hip_int8_set_scales: " + std::to_string(n) + " scales given, the engine has " + std::to_string(e->plan.n_q) +
             " quantized tensors";
    return 1;
  }
  for (int i = 0; i < n; ++i)
    if (!(scales[i] >= 0.0f) || !std::isfinite(scales[i])) { e->err = "p3hip_int8_set_scales: bad scale"; return 1; }
  if (!e->bind()) return 1;
  // the running maxima restart from the loaded calibration: a later p3hip_int8_calibrate widens it
  std::vector<float> amax(n);
  for (int i = 0; i < n; ++i) { e->h_scale[i] = scales[i]; amax[i] = scales[i] * 127.0f; }
  if (!e->check(hipMemcpyAsync(e->d_ascale, e->h_scale.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream), "H2D scales") ||
      !e->check(hipMemcpyAsync(e->d_amax, amax.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream), "H2D amax") ||
      !e->check(hipStreamSynchronize(e->stream), "sync")) return 1;
  e->have_scales = true;
  return 0;
}

int p3hip_upload(p3hip_engine* e) {
  if (!e->bind()) return 1;
  int n = gather_loaded(e);
  if (n == 0) return 0;
  if (!stage_gathered(e, n)) return 1;
  return upload(e, n) && e->check(hipStreamSynchronize(e->stream), "sync") ? 0 : 1;
}

int p3hip_forward_resident(p3hip_engine* e, int n_positions) {
  if (n_positions < 1 || n_positions > e->batch || !e->bind() || !int8_ready(e)) return 1;
  ++e->run_seq;   // d_out is overwritten without a gather: the last p3hip_score no longer answers for the slots
  return run_pass(e, Pass{upload_buffer(e), n_positions, e->d_out}) ? 0 : 1;
}

int p3hip_sync(p3hip_engine* e) { return e->bind() && e->check(hipStreamSynchronize(e->stream), "sync") ? 0 : 1; }

// p3hip_run with the cache on: probe, evaluate the misses only, fill the hits from the table, store the misses.
// d_out / h_out rows: the misses first (in row order), then the hits (in row order); cache.out_row maps.
static int run_cached(p3hip_engine* e, int n) {
  auto& c = e->cache;
  hipStream_t s = e->stream;
  const size_t B = (size_t)e->batch;
  ++c.run;
  if (!upload(e, n) ||   // (the cache's runs are never feats_identity: the upload comes from h_feats_compact)
      !e->check(hipMemcpyAsync(c.d_keys, c.h_keys, (size_t)n * sizeof(p3::CacheKey), hipMemcpyHostToDevice, s), "H2D keys")) return 1;
  p3::CacheArgs a{};
  a.keys = c.d_keys; a.n = n; a.tkeys = c.d_tkeys; a.tmeta = c.d_tmeta; a.tvals = c.d_tvals; a.mask = c.mask; a.run = c.run;
  a.hit = c.d_hit; a.victim = c.d_victim; a.out = e->d_out; a.out_sym = c.d_sym;
  if (!e->check(p3::launch_cache_probe(a, s), "launch k_cache_probe") ||
      !e->check(hipMemcpyAsync(c.h_hit, c.d_hit, (size_t)n * 4, hipMemcpyDeviceToHost, s), "D2H hits") ||
      !e->check(hipMemcpyAsync(c.h_victim, c.d_victim, (size_t)n * 4, hipMemcpyDeviceToHost, s), "D2H victims") ||
      !e->check(hipStreamSynchronize(s), "sync")) return 1;
  int* miss_rows = c.h_lists;
  int* hit_idx = c.h_lists + B;
  int* ins_rows = c.h_lists + 2 * B;
  int* ins_src = c.h_lists + 3 * B;
  int* ins_idx = c.h_lists + 4 * B;
  int nm = 0, nh = 0, ni = 0;
  for (int r = 0; r < n; ++r) nm += c.h_hit[r] < 0;
  int mi = 0, hi = 0;
  std::vector<unsigned char> miss_mask;   // P3HIP_FLAG_SYMMETRY_SLOT: the masks of the misses, by miss row
  // entries this run reads (hits) or has already given to an insert: one writer per entry, no reader evicted
  std::unordered_set<int> claimed;
  for (int r = 0; r < n; ++r) if (c.h_hit[r] >= 0) claimed.insert(c.h_hit[r]);
  for (int r = 0; r < n; ++r) {
    const bool keyed = (c.h_keys[r].lo | c.h_keys[r].hi) != 0;
    c.lookups += keyed;
    if (c.h_hit[r] >= 0) {
      c.was_hit[r] = 1;
      c.out_row[r] = nm + hi;
      hit_idx[hi++] = c.h_hit[r];
      ++c.hits;
    } else {
      c.was_hit[r] = 0;
      c.out_row[r] = mi;
      c.h_sym[mi] = (unsigned)c.h_keys[r].sym;
      miss_rows[mi] = r;
      if (e->sym_slot) miss_mask.push_back(e->row_mask[r]);
      const int v = c.h_victim[r];
      if (keyed && v >= 0 && claimed.insert(v).second) {
        ins_rows[ni] = r; ins_src[ni] = mi; ins_idx[ni] = v; ++ni;
      }
      ++mi;
    }
  }
  nh = hi;
  if (!e->check(hipMemcpyAsync(c.d_lists, c.h_lists, 5 * B * 4, hipMemcpyHostToDevice, s), "H2D lists")) return 1;
  if (nm > 0) {
    a.rows = c.d_lists; a.m = nm; a.feats_in = upload_buffer(e); a.feats_out = c.d_feats2;
    // the misses are evaluated into their d_out rows 0 .. nm - 1 (symmetry averaging: expanded, evaluated and reduced;
    // the stream is drained, so the pinned table is free to take the misses' masks: a subset of the run's, within capacity)
    if ((e->sym_slot && !stage_sym_table(e, miss_mask.data(), nm)) ||
        !e->check(p3::launch_cache_gather(a, s), "launch k_cache_gather") || !run_pass(e, Pass{c.d_feats2, nm, e->d_out}))
      return 1;
  }
  if (nh > 0) {
    a.idx = c.d_lists + B; a.m = nh; a.out_row0 = nm;
    if (!e->check(p3::launch_cache_fill(a, s), "launch k_cache_fill")) return 1;
  }
  if (ni > 0) {
    a.rows = c.d_lists + 2 * B; a.src = c.d_lists + 3 * B; a.idx = c.d_lists + 4 * B; a.m = ni;
    if (!e->check(p3::launch_cache_insert(a, s), "launch k_cache_insert")) return 1;
    c.inserts += ni;
  }
  if (!download(e, n, nullptr)) return 1;
  if (nh > 0 && !e->check(hipMemcpyAsync(c.h_sym + nm, c.d_sym + nm, (size_t)nh * 4, hipMemcpyDeviceToHost, s), "D2H symmetries")) return 1;
  if (!e->check(hipStreamSynchronize(s), "sync")) return 1;
  // P3HIP_FLAG_SYMMETRY_SLOT: the table on the device is the misses'; d_sfeats holds the run's n slots, so put their
  // table back for p3hip_forward_resident and p3hip_time_trunk_kernel (drained again: the next stage reuses the pinned block)
  if (e->sym_slot && nm > 0 && nm < n &&
      (!stage_sym_table(e, e->row_mask.data(), n) || !e->check(hipStreamSynchronize(s), "sync"))) return 1;
  return 0;
}

int p3hip_run(p3hip_engine* e) {
  if (!e->bind() || !int8_ready(e)) return 1;
  int n = gather_loaded(e);
  if (n == 0) return 0;
  if (!stage_gathered(e, n)) return 1;   // (with the cache on: the capacity check over all rows; the misses get their own table)
  if (e->cache.on && !e->calibrating) return run_cached(e, n);   // calibration evaluates every slot, stores nothing
  if (!upload(e, n)) return 1;
  // The heads kernel writes the result records (the first kResultFloats of an output row) a second time into a dense
  // device buffer (HeadsArgs::res), so the copy TrtEngineImpl::RunInference queues behind its graph (trt_engine.cc:283-297)
  // is one contiguous 7.7 MB transfer at the link's rate; the strided copy of rounds 1-3 (1024 rows of 7,556 B out of a
  // 13,664 B pitch) took 0.45 ms, and 4-byte stores straight into host memory from the kernel took as long (round 4,
  // gpurun_out/r4d/breakdown.log).  P3HIP_NO_DIRECT_RESULTS=1: the strided copy (A/B, tests).
  // P3HIP_TIME_RUN=1 (tools/gpu_run_breakdown.py): the stream is drained after every stage and the stages' wall times are
  // summed into the engine's error string on request — a measurement aid, never set in production
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto t_start = now();
  if (e->opt.time_run) {
    hipStreamSynchronize(e->stream);
    e->t_h2d += std::chrono::duration<double>(now() - t_start).count();
    t_start = now();
  }
  const Pass p{upload_buffer(e), n, e->d_out, e->opt.direct_results ? e->d_res : nullptr};   // symmetry: k_sym_reduce fills d_res
  const bool ok = run_pass(e, p);
  if (e->opt.time_run) {
    hipStreamSynchronize(e->stream);
    e->t_fwd += std::chrono::duration<double>(now() - t_start).count();
    t_start = now();
  }
  if (!ok || !download(e, n, p.res)) return 1;
  const bool sync_ok = e->check(hipStreamSynchronize(e->stream), "sync");
  if (e->opt.time_run) {
    e->t_d2h += std::chrono::duration<double>(now() - t_start).count();
    ++e->t_runs;
    char buf[200];
    snprintf(buf, sizeof buf, "timing: runs %ld  h2d %.1f us  forward %.1f us  d2h %.1f us", e->t_runs, e->t_h2d / e->t_runs * 1e6,
             e->t_fwd / e->t_runs * 1e6, e->t_d2h / e->t_runs * 1e6);
    e->err = buf;
  }
  return sync_ok ? 0 : 1;
}

int p3hip_get_slot(p3hip_engine* e, int slot, p3hip_result* out) {
  if (slot < 0 || slot >= e->batch) return 1;
  int row = e->out_row_of(slot);
  if (row < 0) return 2;
  const float* r = e->h_out + (size_t)row * p3::kResultFloats;
  memcpy(out->move_logits, r + p3::kOffMoveLogits, 362 * 4);
  memcpy(out->move_probs, r + p3::kOffMoveProbs, 362 * 4);
  memcpy(out->value_probs, r + p3::kOffValueProbs, 2 * 4);
  memcpy(out->score_probs, r + p3::kOffScoreProbs, 800 * 4);
  memcpy(out->opt_move_probs, r + p3::kOffOptProbs, 362 * 4);
  out->err2_outcome = r[p3::kOffErr2];
  e->slots.fetched(slot);
  return 0;
}

int p3hip_get_slot_keyed(p3hip_engine* e, int slot, p3hip_result* out, int* symmetry, int* from_cache) {
  if (slot < 0 || slot >= e->batch) return 1;
  const int row = e->slots.row(slot), orow = e->out_row_of(slot);
  if (row < 0) return 2;
  if (symmetry) *symmetry = e->cache.on ? (int)e->cache.h_sym[orow] : (int)e->row_sym[row];
  if (from_cache) *from_cache = e->cache.on ? e->cache.was_hit[row] : 0;
  return p3hip_get_slot(e, slot, out);
}

int p3hip_get_ownership(p3hip_engine* e, int slot, float out[P3HIP_NUM_LOCS]) {
  if (slot < 0 || slot >= e->batch) return 1;
  int row = e->out_row_of(slot);
  if (row < 0) return 2;
  if (!e->bind()) return 1;
  if (!e->check(hipMemcpy(out, e->d_out + (size_t)row * p3::kOutStride + p3::kOffOwnership,
                          kNLoc * 4, hipMemcpyDeviceToHost), "D2H ownership")) return 1;
  e->slots.fetched(slot);
  return 0;
}

int p3hip_get_raw(p3hip_engine* e, int slot, float* out) {
  if (slot < 0 || slot >= e->batch) return 1;
  int row = e->out_row_of(slot);
  if (row < 0) return 2;
  std::vector<float> rec(p3::kOutStride);
  if (!e->bind()) return 1;
  if (!e->check(hipMemcpy(rec.data(), e->d_out + (size_t)row * p3::kOutStride, p3::kOutStride * 4,
                          hipMemcpyDeviceToHost), "D2H raw")) return 1;
  memcpy(out, rec.data() + p3::kOffMoveLogits, 362 * 4);
  memcpy(out + 362, rec.data() + p3::kOffOptLogits, 362 * 4);
  memcpy(out + 724, rec.data() + p3::kOffOutcomeLogits, 2 * 4);
  memcpy(out + 726, rec.data() + p3::kOffScoreLogits, 800 * 4);
  memcpy(out + 1526, rec.data() + p3::kOffOwnership, 361 * 4);
  out[1887] = rec[p3::kOffErr2];
  out[1888] = rec[p3::kOffGamma];
  return 0;
}

int p3hip_get_aux(p3hip_engine* e, int slot, float out[P3HIP_AUX_LEN]) {
  if (!(e->flags & P3HIP_FLAG_AUX) || slot < 0 || slot >= e->batch) return 1;
  const int row = e->out_row_of(slot);
  // (a pass stopped in front of the heads, P3HIP_DEBUG_STOP_BLOCK = 0 .. the block count, computes no record)
  const int stop = e->opt.stop_block;
  if (row < 0 || (stop >= 0 && stop <= (int)e->plan.blocks.size())) return 2;
  if (!e->bind()) return 1;
  return e->check(hipMemcpy(out, e->d_aux + (size_t)row * p3::kAuxStride, p3::kAuxFloats * 4, hipMemcpyDeviceToHost),
                  "D2H aux") ? 0 : 1;
}

void p3hip_flops_per_position(const p3hip_engine* e, double* total, double* conv3x3) {
  const WeightFile& w = e->wf;
  const double C = w.model_C, Cb = w.model_Cb, H = w.H, V = w.V, L = kNLoc;
  double mac = L * 25 * 15 * C + 8 * C, mac3 = 0;
  for (int i = 0; i < w.nblocks; ++i) {
    if (is_tfm(e->trunk_path())) mac += L * 4 * C * C + 2 * L * L * C + L * 3 * C * 2 * C;   // q k v o, q.k^T and p.v, SwiGLU
    else if (w.is_broadcast(i)) mac += L * 2 * C * C + C * L * L;
    else if (w.btype == 0) { mac += L * 2 * C * Cb; mac3 += L * w.inner * 9 * Cb * Cb; }
    else if (w.btype == 1) { mac += L * 2 * C * Cb; mac3 += L * 4 * 9 * Cb * Cb; }
    else { mac3 += L * w.inner * 9 * C * C; }
  }
  mac += L * 3 * C * H + L * H * 5 + 2 * H * H + 2 * H * 4 + 2 * H * V * 2 + V * (14 + 51 + 1) +
         (2 * H + 1) * V + 800 * V;
  if (total) *total = 2.0 * (mac + mac3);
  if (conv3x3) *conv3x3 = 2.0 * mac3;
}

double p3hip_time_trunk_kernel(p3hip_engine* e, int n_positions, int iters,
                               double* flops_per_launch, const char** kernel_name) {
  const WeightFile& wf = e->wf;
  const Path path = e->trunk_path();
  int fused_kind = 0, nfused = 0, n3x3 = 0, c3 = 0, nlw = 0;
  for (const BlockPlan& b : e->plan.blocks) {
    if (b.kind == 0 || b.kind == 1) { fused_kind = b.kind; ++nfused; }   // fused block kernel
    if (b.kind == 4) {
      ++nlw;
      for (const LayerPlan& lp : b.layers)
        if (lp.kw == 3) { ++n3x3; c3 = lp.cin; }
    }
  }
  if (n_positions < 1 || n_positions > e->batch || iters < 1 || !e->bind() || !int8_ready(e)) return -1.0;
  ++e->run_seq;   // as p3hip_forward_resident
  // The timed kernel (enqueue_forward records an event pair around each of its launches) and its launches per forward
  // pass: the attention kernel of transformer trunks, the block kernel (k_block, k_blockw; k_block_i8: one launch per
  // btl block), or else the 3x3 layer conv of the layer-wise trunks
  int per_pass = n3x3;
  if (is_tfm(path)) per_pass = wf.nblocks;
  else if (path == Path::Fused || path == Path::Blockw) per_pass = nfused;
  else if (is_int8_fused(path)) per_pass = nlw;
  if (per_pass == 0) return -1.0;
  if (e->any_sym()) {
    // symmetry averaging: the trunk runs over the copies of the resident slots (p3hip_upload put them in d_sfeats)
    if (!expand_sym(e, e->d_sfeats, n_positions)) return -1.0;
    n_positions = e->sym_slot ? sym_rows_of(e, n_positions) : n_positions * e->sym_k;
  }
  while ((int)e->blk_ev.size() < 2 * per_pass) {
    hipEvent_t ev;
    if (!e->check(hipEventCreate(&ev), "hipEventCreate")) return -1.0;
    e->blk_ev.push_back(ev);
  }
  // Time the kernel where it runs: whole forward passes over the resident batch, with a HIP event pair (on the engine's
  // stream) around each timed launch.  The average over all launches is what rocprofv3 --kernel-trace --stats reports
  // for the same run.
  Pass p{e->d_feats, n_positions, e->any_sym() ? e->d_cout : e->d_out};
  if (!enqueue_forward(e, p)) return -1.0;   // warm-up
  double total_ms = 0.0;
  long launches = 0;
  for (int i = 0; i < iters; ++i) {
    int timed = 0;
    p.timed = &timed;
    if (!enqueue_forward(e, p) || !e->check(hipStreamSynchronize(e->stream), "sync")) return -1.0;
    for (int b = 0; b < timed; ++b, ++launches) {
      float ms = 0;
      hipEventElapsedTime(&ms, e->blk_ev[2 * b], e->blk_ev[2 * b + 1]);
      total_ms += ms;
    }
  }
  double flops = 0.0;
  const char* name = nullptr;
  // a 3x3 layer conv
  const double own3 = wf.btype == 2 ? wf.model_C : wf.model_Cb;
  const double conv3 = 2.0 * n_positions * kNLoc * 9.0;
  // every conv of one btl / nbt block: the inner 3x3s plus the 1x1 reduce and expand
  const double n3 = (wf.btype == 0) ? wf.inner : 4;
  const double block_macs = n3 * 9.0 * wf.Cb * wf.Cb + 2.0 * wf.C * wf.Cb;
  switch (path) {
    case Path::Tfm:
    case Path::TfmF32:
    case Path::TfmSplit:
      // q.k^T and p.v over the 361 x 361 tokens of every head (algorithmic, not the padded 384 keys)
      flops = 2.0 * n_positions * 2.0 * kNLoc * kNLoc * wf.model_C;
      name = path == Path::TfmF32 ? p3::tfm_attn_f32_kernel_name() : "k_tfm_attn";
      if (path == Path::TfmSplit) {   // the attention launch of the split in force for these positions
        int parts = 1, tokens = 64;
        tfm_split_of(e, n_positions, &parts, &tokens);
        if (parts > 1) name = "k_tfm_attn_split";
      }
      break;
    case Path::Int8Fused256:
    case Path::Int8Fused128:
      flops = 2.0 * n_positions * kNLoc * block_macs;
      name = p3::block_i8_kernel_name(wf.C);
      break;
    case Path::F32Conv:
    case Path::ConvAny:
    case Path::Split:
    case Path::Int8Any:
    case Path::Int8Conv3:
    case Path::Winograd3:
    case Path::Int8:
    case Path::Layerwise: {
      // the runtime-width kernels: the file's own width, not the padded one the kernel runs; the templated: the layer's
      const LayerKernel lk = layer_kernel(e);
      const double w3 = lk == LayerKernel::Lconv || lk == LayerKernel::LconvI8 ? c3 : own3;
      flops = conv3 * w3 * w3;
      name = layer_kernel_name(lk, 3, c3, c3);
      break;
    }
    case Path::Fused:
    case Path::Blockw: {
      // a launch covers `nfused / launches-per-forward` blocks on average
      const double blocks_per_launch = launches ? (double)nfused * iters / launches : 1.0;
      // plus the broadcast blocks' C -> C convs that ride in the block launches
      int nbconv = 0;
      for (const BlockPlan& b : e->plan.blocks) nbconv += (b.head_of >= 0) + (b.tail_of >= 0);
      const double bconv_per_launch = launches ? (double)nbconv * iters / launches : 0.0;
      // ... and their dense where it rides in the tail (algorithmic 361 x 361 per channel, not the padded K = 384)
      int ndense = 0;
      for (const BlockPlan& b : e->plan.blocks) ndense += b.kind == 3 && b.first_fused && b.dense_fused;
      const double dense_per_launch = launches ? (double)ndense * iters / launches : 0.0;
      flops = 2.0 * n_positions * kNLoc *
              (blocks_per_launch * block_macs + bconv_per_launch * (double)wf.C * wf.C + dense_per_launch * (double)wf.C * kNLoc);
      name = path == Path::Blockw ? (wf.inner == 3 ? "k_blockw_L3" : wf.inner == 2 ? "k_blockw_L2" : "k_blockw_L1")
                                  : p3::block_kernel_name(wf.C, fused_kind, wf.inner);
      break;
    }
    case Path::Refused: break;
  }
  if (flops_per_launch) *flops_per_launch = flops;
  if (kernel_name) *kernel_name = name;
  return launches ? total_ms / launches : -1.0;
}

// debugging aid: the residual stream x of the last forward pass, n_positions x C x 361 fp16 in the device layout
// [pos][C / 8][361][8], as floats
int p3hip_debug_x(p3hip_engine* e, float* out, int n_positions) {
  if (e->any_sym()) { e->err = "p3hip_debug_x: not available on a P3HIP_FLAG_SYMMETRY_AVG / P3HIP_FLAG_SYMMETRY_SLOT engine"; return 1; }
  if (!e->bind() || n_positions < 1 || n_positions > e->batch) return 1;
  return read_acts(e, e->d_x, 0, (size_t)n_positions * e->wf.C * kNLoc, out);
}

// test hook (INT8 layer-wise engines): the int8 activated copy q(mish(bn0(x))) that the last layer-wise block of the pass
// stored for the block behind it (LayerPlan region 3, d_u), [pos][C / 16][361][16]
int p3hip_debug_act_i8(p3hip_engine* e, int8_t* out, int n_positions) {
  const Path path = e->trunk_path();
  if ((path != Path::Int8 && path != Path::Int8Any) || e->any_sym()) {
    e->err = "p3hip_debug_act_i8: only on a P3HIP_FLAG_INT8 / P3HIP_FLAG_INT8_ANY layer-wise engine without P3HIP_FLAG_SYMMETRY_AVG / P3HIP_FLAG_SYMMETRY_SLOT";
    return 1;
  }
  if (!e->bind() || n_positions < 1 || n_positions > e->batch) return 1;
  hipStreamSynchronize(e->stream);
  return e->check(hipMemcpy(out, e->d_u, (size_t)n_positions * e->wf.C * kNLoc, hipMemcpyDeviceToHost), "D2H act") ? 0 : 2;
}

// test hook: what the last transformer block that ran left in HBM, as floats.  which 0, 1, 2: q, k, v of d_qkv,
// [pos][head][384][D] with the 23 padding rows; 3: o of d_t, [pos][361][d].  Only reads; no launch, no allocation on the
// device.  The heads take d_t as scratch, so o is that of the last block only on an engine stopped in front of them
// (P3HIP_DEBUG_STOP_BLOCK = the block count, or any earlier block).
int p3hip_debug_tfm(p3hip_engine* e, int which, float* out, int n_positions) {
  if (!is_tfm(e->trunk_path()) || e->any_sym()) {
    e->err = "p3hip_debug_tfm: only on a transformer engine without P3HIP_FLAG_SYMMETRY_AVG / P3HIP_FLAG_SYMMETRY_SLOT";
    return 1;
  }
  if (which < 0 || which > 3) { e->err = "p3hip_debug_tfm: which must be 0 (q), 1 (k), 2 (v) or 3 (o)"; return 1; }
  if (n_positions < 1 || n_positions > e->last_npos) { e->err = "p3hip_debug_tfm: more positions than the last run had"; return 1; }
  if (!e->bind()) return 1;
  const size_t d = (size_t)e->wf.model_C;
  const size_t per = (size_t)e->rows * p3::kTfmLPad * d;
  const size_t n = (size_t)n_positions * (which < 3 ? p3::kTfmLPad : kNLoc) * d;
  return which < 3 ? read_acts(e, e->d_qkv, which * per, n, out) : read_acts(e, e->d_t, 0, n, out);
}

// test hook: every value buffer a forward pass (or p3hip_score / p3hip_loss) must define before it reads it, filled with
// `byte` on the engine's stream: the rows of kDeviceBuffers of class Poisoned, and of a ZeroedOnce buffer what lies outside
// its zero range.  State and Index buffers are left alone, so no later run can compute an address from the fill.  The
// results of earlier runs are gone: no slot keeps a row and the rows count as overwritten (run_seq), as after the hooks
// that write d_out without a gather.  No pointer changes, so a captured graph stays valid.
int p3hip_debug_poison(p3hip_engine* e, int byte) {
  if (byte < 0 || byte > 255) { e->err = "p3hip_debug_poison: the fill is one byte, 0 .. 255"; return 1; }
  if (!e->bind()) return 1;
  for (const DeviceBuffer& b : kDeviceBuffers) {
    void* p = b.ptr(e);
    if (!p) continue;
    if (b.cls == BufClass::Poisoned && !e->check(hipMemsetAsync(p, byte, b.bytes(e), e->stream), b.name)) return 1;
    if (b.cls == BufClass::ZeroedOnce && !b.poison_rest(e, byte)) return 1;
  }
  if (!e->check(hipStreamSynchronize(e->stream), "sync")) return 1;
  ++e->run_seq;   // p3hip_score, p3hip_loss and their getters stop answering for the last run
  e->slots.drop_rows();   // p3hip_get_*: 2, not evaluated (a slot not yet fetched stays pending for the next run)
  return 0;
}

// test hook, no device needed: the table p3hip_debug_poison goes by, one line per device pointer member of p3hip_engine,
// "name<TAB>class<TAB>the range that stays zero (zeroed-once only)"
const char* p3hip_debug_poison_table(void) {
  static const std::string text = [] {
    std::string t;
    for (const DeviceBuffer& b : kDeviceBuffers) t += std::string(b.name) + "\t" + class_name(b.cls) + "\t" + b.zero_range + "\n";
    return t;
  }();
  return text.c_str();
}

void p3hip_rope_table(double* cos_out, double* sin_out) { spiral_rope_table(32, cos_out, sin_out); }

int p3hip_rope_table_dim(int head_dim, double* cos_out, double* sin_out) {
  if (head_dim != 32 && head_dim != 64) return 1;
  spiral_rope_table(head_dim, cos_out, sin_out);
  return 0;
}

void p3hip_symmetry_maps(uint16_t fwd[8][361], uint16_t inv[8][361]) { p3::sym_maps(fwd, inv); }

int p3hip_debug_symmetry_rows(const uint8_t* masks, int n, int rows, int* first, int* total) {
  return p3::sym_rows(masks, n, rows, first, total);
}

int p3hip_set_slot_symmetries(p3hip_engine* e, int slot, uint32_t mask) {
  if (!e->sym_slot) { e->err = "p3hip_set_slot_symmetries: the engine was not created with P3HIP_FLAG_SYMMETRY_SLOT"; return 1; }
  if (slot < 0 || slot >= e->batch) { e->err = "p3hip_set_slot_symmetries: bad slot"; return 1; }
  if (mask < 1 || mask > 255) { e->err = "p3hip_set_slot_symmetries: the mask must be 1 .. 255 (bit s = symmetry s)"; return 1; }
  e->slot_mask[slot] = (unsigned char)mask;
  return 0;
}

int p3hip_set_symmetries(p3hip_engine* e, uint32_t mask) {
  if (!e->sym) { e->err = "p3hip_set_symmetries: the engine was not created with P3HIP_FLAG_SYMMETRY_AVG"; return 1; }
  if (mask < 1 || mask > 255) { e->err = "p3hip_set_symmetries: the mask must be 1 .. 255 (bit s = symmetry s)"; return 1; }
  if (mask == e->sym_mask) return 0;
  if (!e->bind()) return 1;
  // the captured graph holds the old list in its kernel arguments: drop it.  The next full run goes out kernel by
  // kernel (a new k means new row counts, whose launchers may meet kernels for the first time), the one after is captured
  // (P3HIP_FLAG_LAUNCH_GRAPH_ANY: every graph of the table and every sighting, so each key starts again the same way)
  if ((e->graph_exec || e->graph || e->graph_table.held() > 0) && !e->check(hipStreamSynchronize(e->stream), "sync")) return 1;
  drop_graph(e);
  e->graph_warm = false;
  e->sym_mask = mask;
  e->sym_k = p3::sym_list(mask, e->sym_syms);
  return 0;
}

int p3hip_blockw_stamps(p3hip_engine* e, unsigned long long* out, int n) {
  if (!e->bind() || !e->d_bw_stamps) return 1;
  constexpr int total = 8 * 16 * 4 * 24;
  hipStreamSynchronize(e->stream);
  return hipMemcpy(out, e->d_bw_stamps, (size_t)(n < total ? n : total) * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}

#ifdef P3_DIAG
// diagnostic build only: the phase stamps of the last forward pass's launch P3DIAG_LAUNCH
int p3hip_debug_block_stamps(p3hip_engine* e, unsigned long long* out, int n) {
  if (!e->bind() || !e->d_stamps) return 1;
  constexpr int total = p3::kStampWgs * 8 * p3::kStampSections * p3::kStampSlots;
  hipStreamSynchronize(e->stream);
  return hipMemcpy(out, e->d_stamps, (size_t)(n < total ? n : total) * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}
int p3hip_debug_block_spans(p3hip_engine* e, unsigned long long* out, int n) {
  if (!e->bind() || !e->d_spans) return 1;
  constexpr int total = p3::kSpanWgs * p3::kSpanSlots;
  hipStreamSynchronize(e->stream);
  return hipMemcpy(out, e->d_spans, (size_t)(n < total ? n : total) * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 2;
}
#endif

}  // extern "C"
