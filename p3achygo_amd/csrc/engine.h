// engine.h — struct p3hip_engine, shared by engine.cpp (the C ABI: create / destroy, slots, cache, calibration, timing and
// debug entry points) and forward.cpp (the forward pass).  Internal: include/p3hip.h is the interface.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/p3hip.h"
#include "graph_table.h"
#include "heads_aux.h"
#include "kernels.h"
#include "plan.h"
#include "slot_state.h"
#include "symmetry.h"

namespace eng {

constexpr size_t kFeatBytes = sizeof(p3hip_features);
static_assert(sizeof(p3hip_features) == 1860, "p3hip_features layout");
static_assert(sizeof(p3hip_result) == 4 * 1892, "p3hip_result layout");

// One forward pass: everything it reads or writes that changes from call to call.
struct Pass {
  const unsigned char* feats = nullptr;   // the records k_init reads (a symmetry pass: the records k_sym_expand reads)
  int npos = 0;
  float* out = nullptr;   // the rows the heads write: d_out, or d_cout for the copies of a symmetry pass
  float* res = nullptr;   // d_res: the result records a second time, dense (HeadsArgs::res); null: not written
  int* timed = nullptr;   // p3hip_time_trunk_kernel: launches timed so far, event pairs e->blk_ev[2 i, 2 i + 1]
};

// P3HIP_FLAG_LAUNCH_GRAPH_ANY: one captured pass of the engine's table (p3hip_engine::graph_slots)
struct GraphSlot {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
};

}  // namespace eng

struct p3hip_engine {
  std::string path, err;
  int batch = 0, device = 0;
  uint32_t flags = 0;
  eng::WeightFile wf;
  eng::Options opt;   // the P3HIP_* environment switches, as p3hip_create found them
  eng::Plan plan;     // the trunk path (plan.choice.path: everything switches on it) and the arena offsets
  int n_cu = 256;
  int last_npos = 0;       // positions of the last forward pass enqueued or replayed (p3hip_debug_tfm)
  // k_blockw (csrc/asm/blockw_gen.py): the module of the hand-scheduled one-wave-per-SIMD kernel, loaded on first use
  hipModule_t bw_mod = nullptr;
  hipFunction_t bw_fn = nullptr;
  unsigned long long* d_bw_stamps = nullptr;   // P3HIP_BLOCKW_DIAG: s_memtime stamps of the _diag kernel
  hipStream_t stream = nullptr;
  // P3HIP_FLAG_LAUNCH_GRAPH: the forward pass over the full static batch, captured once (trt_engine.cc:260-303)
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  bool graph_failed = false, graph_warm = false;
  eng::Pass graph_pass;   // the pass the graph was captured for (kernel arguments are baked in): its feats and res are the key
  uint64_t graph_captures = 0, graph_replays = 0, graph_launched = 0;   // p3hip_graph_stats of that one graph
  // P3HIP_FLAG_LAUNCH_GRAPH_ANY: a graph per key (slots, forward rows, feature buffer, result
  // target).  graph_table (graph_table.h) decides what a pass does and hands out the slots of graph_slots, which holds
  // the graphs; graph_seq counts the passes the table saw (the tags of its entries)
  gt::Table graph_table;
  std::vector<eng::GraphSlot> graph_slots;
  long graph_seq = 0;
  bool graph_any() const { return (flags & P3HIP_FLAG_LAUNCH_GRAPH_ANY) != 0; }
  // p3hip_time_trunk_kernel: event pairs around the timed launches of a forward pass
  std::vector<hipEvent_t> blk_ev;

  // Every device pointer below (d_*, those of the nested structs included) has one row in kDeviceBuffers (engine.cpp): its
  // size and whether a forward pass may read what an earlier one left there.  A new buffer needs a row, or
  // tests/test_scratch_poison_cpu.py fails.
  unsigned char* d_arena = nullptr;
  size_t arena_bytes = 0;
  p3::HeadsArgs heads_args{};   // the heads' weight pointers, set once at create; a pass fills x, hp, out, res and npos
  // The INT8 paths: the layer-wise blocks' convs run on int8 inputs with per-tensor activation
  // scales.  amax: running per-tensor maxima of the calibration runs (float bits, atomicMax); scale: the s_a = max / 127
  // the int8 kernels read at launch time, so that a replayed graph sees new scales.  Int8Fused256 / Int8Fused128
  // ("Fused INT8 blocks"): the btl blocks are planned layer by layer (the fp16 plan the calibration runs, at C = 128
  // through k_lconv_any) and run as one k_block_i8 launch each (block_i8.hip, one kernel at two geometries).
  bool calibrating = false, have_scales = false;
  unsigned* d_amax = nullptr;
  float* d_ascale = nullptr;
  std::vector<float> h_scale;
  // P3HIP_FLAG_SYMMETRY_AVG: every slot is evaluated as k copies, one per symmetry of the mask,
  // and the rows averaged back into d_out.  rows: the row capacity of the per-row device buffers (8 x batch with the
  // flag, batch without).  The upload lands in d_sfeats, k_sym_expand writes the copies to d_feats, the heads write the
  // copies' rows to d_cout, k_sym_reduce averages them into d_out (and d_res).
  bool sym = false;
  uint32_t sym_mask = 0xFF;
  int sym_k = 8;
  int sym_syms[p3::kNumSyms] = {0, 1, 2, 3, 4, 5, 6, 7};
  int rows = 0;
  unsigned char* d_sfeats = nullptr;
  float* d_cout = nullptr;
  // P3HIP_FLAG_SYMMETRY_SLOT: the same buffers, with a mask per slot and `rows` = the
  // symmetry_rows of p3hip_create_rows.  slot_mask: by slot (set after the load, reset to 0x01 by every load); row_mask:
  // by dense row of the last gather.  The table of a pass (stage_sym_table: first[] as p3::sym_rows gives it, then the
  // masks, tab_n rows) goes up in one copy: h_symtab is pinned, [batch] ints then [batch] bytes, d_symtab its device
  // twin; tab_first / tab_mask point into d_symtab.  tab_total: the copies of those tab_n rows.
  bool sym_slot = false;
  std::vector<unsigned char> slot_mask, row_mask;
  unsigned char *h_symtab = nullptr, *d_symtab = nullptr;
  int tab_n = 0, tab_total = 0;
  const int* tab_first() const { return reinterpret_cast<const int*>(d_symtab); }
  const unsigned char* tab_mask() const { return d_symtab + (size_t)batch * 4; }
  bool any_sym() const { return sym || sym_slot; }

  // buffers
  unsigned char* h_feats = nullptr;       // pinned [batch] slots as loaded
  unsigned char* h_feats_compact = nullptr;  // pinned, dense
  unsigned char* d_feats = nullptr;
  // The activations.  On the fp32 paths (F32Conv, TfmF32) weights and these buffers are fp32: they keep their fp16
  // pointer types and are eng::act_bytes(path) = 4 bytes per element, and no fp16 value exists in the pass.
  _Float16 *d_x = nullptr, *d_t = nullptr, *d_u = nullptr;
  _Float16* d_qkv = nullptr;   // transformer trunks: q, k, v [3][rows][head][384][D] (rows 361.. zeroed once)
#ifdef P3_DIAG
  unsigned long long* d_stamps = nullptr;   // diagnostic build: k_block phase stamps of one launch (P3DIAG_LAUNCH)
  unsigned long long* d_spans = nullptr;    // and every workgroup's entry / per-position / exit times of that launch
  int launch_index = 0;
#endif
  _Float16* d_s = nullptr;   // nbt trunks: the block kernel's inner-stream scratch (t and u carry the broadcast blocks' tensors)
  float* d_hp = nullptr;
  float* d_pool = nullptr;   // Split, TfmSplit: what the split heads pool per row, [rows][p3::kHeadsPoolFloats] (edge_split.h)
  // P3HIP_FLAG_AUX: k_heads_aux writes one record per row of the pass into d_aux [rows][kAuxStride],
  // allocated under the flag only; aux_args: its weight pointers, set once at create (a pass fills hp, aux and npos)
  float* d_aux = nullptr;
  p3::HeadsAuxArgs aux_args{};
  float* d_out = nullptr;
  float* h_out = nullptr;  // pinned [batch][kResultFloats]
  float* d_res = nullptr;  // [batch][kResultFloats] dense: the heads kernel writes the result records a second time there
                           // (Pass::res), so that the D2H copy is ONE contiguous transfer instead of a strided one
  double t_h2d = 0, t_fwd = 0, t_d2h = 0;   // P3HIP_TIME_RUN
  long t_runs = 0;
  bool feats_identity = false;   // gather_loaded: every slot was dirty, row == slot: the upload comes straight from h_feats
  p3::SlotStates slots;   // dirty flags + slot -> dense row of the last run (slot_state.h)
  int last_n = 0;
  std::vector<unsigned char> slot_sym, row_sym;   // symmetry given with a keyed load, by slot / by row of the last run

  // on-device NN cache (p3hip_cache_enable): the table, the per-slot keys as loaded, and the per-run lists
  struct DeviceCache {
    bool on = false;
    unsigned mask = 0, run = 0;
    unsigned long long* d_tkeys = nullptr;
    unsigned* d_tmeta = nullptr;
    float* d_tvals = nullptr;
    p3::CacheKey* h_slot_keys = nullptr;   // [batch] by slot (plain memory, written by load_slot_keyed)
    p3::CacheKey *h_keys = nullptr, *d_keys = nullptr;   // [batch] by row of the run (pinned / device)
    int *h_hit = nullptr, *d_hit = nullptr, *h_victim = nullptr, *d_victim = nullptr;
    int *h_lists = nullptr, *d_lists = nullptr;          // [5][batch]: miss rows, hit entries, insert rows, insert src, insert entries
    unsigned *h_sym = nullptr, *d_sym = nullptr;         // [batch] symmetry of the result in out row r
    unsigned char* d_feats2 = nullptr;                   // features of the misses, dense
    std::vector<int> out_row;                            // row of the run -> row of d_out / h_out
    std::vector<unsigned char> was_hit;                  // by row of the run
    unsigned long long lookups = 0, hits = 0, inserts = 0;
  } cache;
  // Scoring against labels (include/p3hip.h; scoring.cpp, score.hip).  The labels live per slot in pinned memory and
  // belong to the slot's current load (has_labels[slot], cleared by p3hip_load_slot*).  p3hip_score gathers those of the
  // last run's rows into h_dense / h_rows (entry k scores output row h_rows[k]), uploads, and reads back terms and sums.
  // The buffers are made by the first p3hip_load_labels (many threads may race for it) or p3hip_debug_score_rows.
  struct Scoring {
    std::mutex mu;
    std::atomic<bool> ready{false};
    p3hip_labels *h_slot = nullptr, *h_dense = nullptr, *d_labels = nullptr;   // pinned [batch] by slot / dense; device
    int *h_rows = nullptr, *d_rows = nullptr;
    float *h_terms = nullptr, *d_terms = nullptr;   // [batch][P3HIP_NUM_SCORE_TERMS]
    double *h_sums = nullptr, *d_sums = nullptr;
    std::vector<int> entry_of_slot;   // slot -> entry of the last p3hip_score (-1: not scored)
    long scored_run = -1;             // run_seq that p3hip_score scored
  } scoring;
  std::vector<unsigned char> has_labels;   // [batch]
  // The validation losses (include/p3hip.h; loss_abi.cpp, loss.hip): the twin of Scoring.  The targets live per slot in
  // pinned memory, packed by p3hip_load_targets into the device layout of loss.h, and belong to the slot's current load
  // (has_targets[slot], cleared by p3hip_load_slot*).  p3hip_loss gathers those of the last run's rows into h_dense /
  // h_rows (entry k: rows h_rows[k] of d_out and d_aux); when entry k is slot k for all of them the upload comes straight
  // from h_slot.  The buffers are made by the first p3hip_load_targets or p3hip_debug_loss_rows.
  struct Loss {
    std::mutex mu;
    std::atomic<bool> ready{false};
    float *h_slot = nullptr, *h_dense = nullptr, *d_targets = nullptr;   // [batch][kTgtStride]: pinned by slot / dense; device
    int *h_rows = nullptr, *d_rows = nullptr;
    float *h_terms = nullptr, *d_terms = nullptr;     // [batch][P3HIP_NUM_LOSS_TERMS]
    double *h_sums = nullptr, *d_sums = nullptr;
    std::vector<int> entry_of_slot;   // slot -> entry of the last p3hip_loss (-1: not handled)
    long loss_run = -1;               // run_seq that p3hip_loss handled
  } loss;
  std::vector<unsigned char> has_targets;   // [batch]
  // load_seq[slot] counts the slot's loads, run_load_seq[slot] is its value when the last run gathered the slot:
  // p3hip_score leaves out a slot that was loaded again since (its labels are the new position's, its row the old one's)
  std::vector<unsigned> load_seq, run_load_seq;
  // counts whatever hands the output rows to someone else: every gather (p3hip_run, p3hip_int8_calibrate, p3hip_upload)
  // and the hooks that write d_out without one (p3hip_forward_resident, p3hip_time_trunk_kernel, p3hip_debug_score_rows)
  long run_seq = 0;
  long gather_seq = 0;   // run_seq of the last gather: while they are equal, d_out still holds that run's rows

  // row of d_out / h_out that holds `slot`'s result (-1: not evaluated by the last run)
  int out_row_of(int slot) const {
    const int row = slots.row(slot);
    return (row >= 0 && cache.on) ? cache.out_row[row] : row;
  }

  eng::Path trunk_path() const { return plan.choice.path; }
  bool check(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    err = std::string(what) + ": " + hipGetErrorString(e);
    return false;
  }
  template <class T>
  const T* dev(size_t off) const { return reinterpret_cast<const T*>(d_arena + off); }
  // HIP's current device is per host thread, and the ABI is called from whatever thread the
  // host likes (the infer thread, one GPU thread per game group, a rank's main thread): every
  // entry point that touches HIP binds the engine's device first.
  bool bind() { return check(hipSetDevice(device), "hipSetDevice"); }
};

namespace eng {

// forward.cpp
// The kernel that runs the convs of the layer-wise blocks in the engine's present state, and its name in a profile
enum class LayerKernel { Lconv, LconvAny, LconvI8, LconvI8Any, LconvF32, Sconv, Wconv };
LayerKernel layer_kernel(const p3hip_engine* e, int kw = 3);   // (kw: of the layer; the timed convs are the 3x3)
const char* layer_kernel_name(LayerKernel k, int kw, int cin, int cout);
void tfm_split_of(const p3hip_engine* e, int npos, int* parts, int* tokens);   // Path::TfmSplit: the split of a launch
// Path::Split, Path::TfmSplit: the parts per position of the stem, broadcast dense and heads launches (edge_split.h)
void edge_split_of(const p3hip_engine* e, int npos, int* stem, int* dense, int* heads);
bool enqueue_forward(p3hip_engine* e, const Pass& p);
bool expand_sym(p3hip_engine* e, const unsigned char* src, int n);
// P3HIP_FLAG_SYMMETRY_SLOT: builds the table of the `n` dense rows with `masks` and queues its upload; false with the
// sum and the capacity in e->err when the copies exceed e->rows (nothing is queued then)
bool stage_sym_table(p3hip_engine* e, const unsigned char* masks, int n);
// the forward rows of the first `n` rows of the staged table (-1: the table holds fewer rows)
int sym_rows_of(const p3hip_engine* e, int n);
bool run_pass(p3hip_engine* e, const Pass& p);
void drop_graph(p3hip_engine* e);
// scoring.cpp
void free_scoring(p3hip_engine* e);
// loss_abi.cpp
void free_loss(p3hip_engine* e);

}  // namespace eng
