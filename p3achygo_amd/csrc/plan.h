// plan.h — the host-side plan of an engine: which trunk path it runs (choose_plan), and the weights of that path repacked
// into one arena image with the offsets the forward pass needs (build_plan).  Nothing here calls the HIP runtime: a bad
// file or a refused flag set fails before any device call, GPU or not.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "graph_table.h"
#include "heads_aux.h"
#include "kernels.h"
#include "weights.h"

namespace eng {

constexpr int kNLoc = 361;

// Every P3HIP_* environment switch of the engine, read once at the top of p3hip_create.
struct Options {
  bool c128_wg8 = false;   // P3HIP_C128_WG8: C = 128 blocks as one 8-wave workgroup per CU (A/B timing)
  bool bcast_fuse = true;  // P3HIP_NO_BFUSE clears it: broadcast 1x1 convs as their own launches (A/B, tests)
  bool dense_fuse = true;  // P3HIP_NO_DFUSE clears it: the broadcast dense as its own launch (k_bdense)
  bool heads_fuse = true;  // P3HIP_NO_HFUSE clears it: the head convs as their own launch in front of k_heads
  int stop_block = -1;     // P3HIP_DEBUG_STOP_BLOCK: the forward pass ends in front of plan block n (debugging, tests)
  bool fuse = true, join = true;   // P3HIP_NO_FUSE clears both: one k_block launch per block; P3HIP_NO_JOIN join: one per run
  int stagger = -1;        // P3HIP_STAGGER: block launches' start-up stagger in cycles (-1: the launch decides)
  bool pair_turns = true;  // P3HIP_NO_PAIR_TURNS clears it: C = 128 workgroup pairs leave the wave priorities alone
  bool direct_results = true;   // P3HIP_NO_DIRECT_RESULTS clears it: p3hip_run copies the results strided from d_out
  bool time_run = false;   // P3HIP_TIME_RUN: p3hip_run times its stages (a measurement aid)
  bool blockw = false;     // P3HIP_BLOCKW=1: C = 256 / C_b = 128 btl runs through k_blockw (csrc/asm/blockw_gen.py)
  bool blockw_diag = false;   // P3HIP_BLOCKW_DIAG: the _diag twin, which writes the engine's d_bw_stamps
  bool conv_any = false;   // P3HIP_CONV_ANY=1: the templated layer-wise shapes through conv_any.hip too (and, with
                           // P3HIP_FLAG_INT8_ANY, through k_lconv_i8_any)
  // P3HIP_SPLIT="S,T" (P3HIP_FLAG_LOW_LATENCY engines; tests, A/B runs): every k_sconv launch splits a position into S row
  // strips and T-channel output tiles.  0, 0: the launch chooses (conv_split.h sconv_split).  split_bad: the variable is
  // set to something else than a pair of the kernel's sets, which fails the creation of such an engine
  int split_s = 0, split_t = 0;
  bool split_bad = false;
  // P3HIP_TFM_SPLIT="S,T" (P3HIP_FLAG_LOW_LATENCY_TFM engines; tests, A/B runs): every launch of a transformer block takes
  // S query parts per (position, head) and T tokens per workgroup.  0, 0: the launch chooses (transformer_split.h
  // tfm_split).  tfm_split_bad: set to something else than a pair of the kernels' sets, which fails such an engine's creation
  int tfm_split_s = 0, tfm_split_t = 0;
  bool tfm_split_bad = false;
  // P3HIP_EDGE_SPLIT="s,d,h" (engines of either low-latency flag; tests, A/B runs): the parts per position of every stem,
  // broadcast dense and heads launch (edge_split.h; s is 1 or the stem's output passes, which depends on the file and is
  // checked by choose_plan).  "0": all three unsplit, 1,1,1.  0, 0, 0: the launch chooses (edge_split).  edge_bad: the
  // variable is set to something else, which fails the creation of such an engine
  int edge_s = 0, edge_d = 0, edge_h = 0;
  bool edge_bad = false;
  // P3HIP_GRAPH_CACHE (P3HIP_FLAG_LAUNCH_GRAPH_ANY engines): the graphs the engine's table holds, 1..1024 (graph_table.h).
  // graph_cache_bad: set to anything else, which fails the creation of such an engine
  int graph_cache = 64;
  bool graph_cache_bad = false;
  // P3HIP_GRAPH_MIN_SEEN, P3HIP_GRAPH_MAX_ROWS (the same engines; A/B runs, tools/gpu_graph_any_ab.py): a key is captured on
  // its n-th sighting (2..64, never the first: graph_table.h), and only a pass of at most so many forward rows is (0: no
  // limit; a pass over the full static batch always is).  Out of range: the nearest bound.  Defaults: graph_table.h
  int graph_min_seen = gt::kMinSeen, graph_max_rows = gt::kDefaultMaxRows;
  static Options from_env();
};

// The trunk path of an engine: the one decision the packers, the buffer sizing, the forward pass, the timing and the
// debug read-backs switch on.
enum class Path {
  Refused,        // choose_plan filled the error text
  Fused,          // k_block: btl and nbt at C = 256 / 128 and 128 / 64, broadcast convs and dense fused into the runs
  Blockw,         // k_blockw runs (P3HIP_BLOCKW) at C = 256 / 128 btl; broadcast blocks as their own launches
  Layerwise,      // templated k_lconv: C = 384 / C_b = 192 btl and nbt, classic C = 192
  ConvAny,        // conv_any.hip, widths as launch arguments: every other trunk of P3HIP_CONV_SET (and P3HIP_CONV_ANY=1)
  Int8,           // P3HIP_FLAG_INT8: k_lconv_i8 on the templated layer-wise shapes
  Int8Fused256,   // P3HIP_FLAG_INT8_FUSED: k_block_i8 per btl block at C = 256 / C_b = 128
  Int8Fused128,   // P3HIP_FLAG_INT8_C128: the same at C = 128 / C_b = 64 (block_i8.hip, geometry <128,64>)
  Int8Any,        // P3HIP_FLAG_INT8_ANY on every trunk the three above do not serve: k_lconv_i8_any, widths as launch
                  // arguments; stem, broadcast blocks and heads as ConvAny's
  Int8Conv3,      // P3HIP_FLAG_INT8_CONV3 on the btl / nbt trunks whose fp16 plan is Layerwise or ConvAny: that plan's layers,
                  // the 3x3 convs through k_lconv_i8 / k_lconv_i8_any, everything else in fp16 (PlanChoice::any_width: the
                  // runtime-width kernels).  A classic trunk has only 3x3 convs and takes Int8 / Int8Any itself
  Winograd3,      // P3HIP_FLAG_WINOGRAD on the trunks whose fp16 plan is Layerwise or ConvAny, classic included: that plan's
                  // layers, arena and buffers, the 3x3 convs through k_wconv (conv_wino.hip) from one more weight image
                  // per 3x3 layer (LayerPlan::wino_off), everything else the fp16 plan's kernels (PlanChoice::any_width)
  F32Conv,        // P3HIP_FLAG_FP32: every conv trunk layer by layer through conv_f32.hip
  Split,          // P3HIP_FLAG_LOW_LATENCY: every conv trunk layer by layer through k_sconv (conv_split.hip), a position
                  // split across workgroups; stem, broadcast dense and heads as ConvAny's
  Tfm,            // transformer trunk, fp16
  TfmF32,         // P3HIP_FLAG_FP32_TFM: transformer trunk through transformer_f32.hip
  TfmSplit,       // P3HIP_FLAG_LOW_LATENCY_TFM: Tfm's arena, stem, heads and buffers; the blocks' launches split across more
                  // workgroups (transformer_split.hip), bit-identical to Tfm
};
inline bool is_tfm(Path p) { return p == Path::Tfm || p == Path::TfmF32 || p == Path::TfmSplit; }
inline bool is_f32(Path p) { return p == Path::F32Conv || p == Path::TfmF32; }
inline bool is_int8_fused(Path p) { return p == Path::Int8Fused256 || p == Path::Int8Fused128; }
// (an INT8 engine calibrates through the fp16 layer-wise plan: `calibrating` is a run-time state of the engine)
inline bool is_int8(Path p) { return p == Path::Int8 || p == Path::Int8Any || p == Path::Int8Conv3 || is_int8_fused(p); }
// conv blocks planned conv by conv (BlockPlan kind 4)
inline bool is_layerwise(Path p) {
  return p == Path::Layerwise || p == Path::ConvAny || is_int8(p) || p == Path::Winograd3 || p == Path::F32Conv || p == Path::Split;
}
inline size_t act_bytes(Path p) { return is_f32(p) ? 4 : 2; }   // bytes per activation element of d_x, d_t, d_u, d_qkv

struct PlanChoice {
  Path path = Path::Refused;
  int CB = 0;    // slice width of the per-position kernels that stage C channels (k_conv1x1 family)
  int CPI = 0;   // output pass width of the init conv
  bool heads_image = false;   // the arena holds k_headsx's weight fragments and tensor image (C <= 256, fp16)
  bool heads_fused = false;   // k_headsx runs: the head convs inside the heads kernel (P3HIP_NO_HFUSE, conv_any clear it)
  int tfm_heads = 0, tfm_D = 0;   // transformer: head count and head width (model width wf.model_C = heads x D)
  bool any_width = false;   // Int8Conv3, Winograd3: the fp16 plan of this trunk is ConvAny's (a padded or runtime width, P3HIP_CONV_ANY=1)
};
// the stem, the broadcast blocks, the head convs and the fp16 layer convs (calibration) through conv_any.hip
// (Split: all of these but the layer convs and the broadcast blocks' two 1x1 convs, which run through k_sconv)
inline bool runs_conv_any(const PlanChoice& c) {
  return c.path == Path::ConvAny || c.path == Path::Int8Any || c.path == Path::Split ||
         ((c.path == Path::Int8Conv3 || c.path == Path::Winograd3) && c.any_width);
}

const char* path_name(Path p);   // "Fused", "Int8Any", ..: the enumerator's name (p3hip_debug_plan)

// Pure: every refusal of an engine's creation that depends on the file's architecture and the flags, in their order of
// precedence, and the path of an engine that is served.
PlanChoice choose_plan(const WeightFile& wf, uint32_t flags, const Options& opt, std::string& err);

// ---- device arena -----------------------------------------------------------------
struct Arena {
  std::vector<unsigned char> host;
  bool bad_stream = false;
  size_t add(const void* p, size_t bytes) {
    size_t off = (host.size() + 255) & ~size_t(255);
    host.resize(off + bytes);
    memcpy(host.data() + off, p, bytes);
    return off;
  }
};

struct FoldedBN { size_t scale_off, shift_off; };

// One conv of a layer-wise block (kind 4), or one of the two 1x1 convs of a broadcast block (kind 3).  Regions: 0 = x;
// 1, 2 = the two C_b-channel halves of the scratch buffer t; 3, 4 = those of u (1 and 3 also name t and u as whole
// C-channel buffers).
struct LayerPlan {
  int kw, cin, cout;
  bool pre;
  int act;                    // 0, 1 = mish(out_bn(y)), 2 = mish(y) (conv_first of a broadcast block)
  bool res, dual;             // see p3::LConvArgs
  FoldedBN pre_bn, out_bn;    // prologue / epilogue BN (epilogue: of act or of dual's second output)
  int in_buf, out_buf, out2_buf;
  // The weight image of the kernel the path runs this conv with: an fp16 stream of nms macro-steps (k_lconv and its
  // runtime-width twin, which the INT8 paths calibrate through; k_conv1x1 on a broadcast block), conv_f32.h
  // pack_conv_f32 (F32Conv) or conv_split.h pack_sconv (Split)
  size_t w_off = 0;
  int nms = 0;
  // INT8 paths: the quantized weights (lconv_i8.h pack_lconv_i8), their per-output-channel scales, and the index of
  // this layer's input among the engine's quantized tensors (its output, when quantized, is the next one: its consumer).
  // Int8Conv3: on the 3x3 layers only; a 1x1 layer in front of one quantizes its output for it
  size_t q_off = 0, qs_off = 0;
  int qidx = -1;
  size_t wino_off = 0;   // Winograd3, 3x3 layers: k_wconv's image (conv_wino.h pack_wconv), behind everything else in the arena
  int out_qidx = -1;   // Int8Conv3: the consumer's qidx where this layer stores its activated output as int8, else -1 (fp16)
};

// One transformer block (kind 5): arena offsets of its tensors, the GEMM weights as MFMA A fragments (transformer.h)
struct TfmPlan { size_t rms_in = 0, rms_out = 0, wqkv = 0, wo = 0, wgu = 0, wdown = 0; };

struct BlockPlan {
  int kind;  // 0 btl, 1 nbt, 3 broadcast, 4 layer-wise, 5 transformer
  TfmPlan tfm;
  // layer-wise: one per conv.  broadcast: conv_first {kw 1, C -> C, pre, act 2, x -> t} and conv_last {res, u -> x}
  std::vector<LayerPlan> layers;
  // fused blocks: the block's stream; the launch picks the macro-step size (kernels.h block_macro_step_bytes)
  size_t stream_off = 0;
  int nms = 0;
  size_t stream_bytes = 0;
  FoldedBN bn[p3::kMaxBlockLayers];
  // broadcast: the dense matrix for the path's kernel (an fp16 stream of dense_nms macro-steps, or conv_f32.h
  // pack_dense_f32) and its bias
  size_t dense_off = 0;
  int dense_nms = 0;
  size_t dense_bias_off = 0;
  // Broadcast 1x1 convs taken into the neighbouring block launches (k_block's BC form).
  //   on a broadcast block: its conv_first runs at the tail of the launch before it / its conv_last
  //   at the head of the launch after it;
  //   on a fused block: the run's first block carries the head conv (head_of = that broadcast block,
  //   its stream lies right before stream_off), the run's last block the tail conv (right after).
  bool first_fused = false, last_fused = false;
  bool dense_fused = false;   // C = 256: the dense runs in that tail as well (no k_bdense launch, t never stored)
  int head_of = -1, tail_of = -1;
  size_t head_bytes = 0, tail_bytes = 0;
  int bw_run = -1;   // Blockw: the k_blockw run (Plan::bw_runs) that starts at this block
};

// The small tensors of the heads (kernels.h HeadsArgs), in the order they are uploaded to the arena.  The one table
// serves the upload, the order of k_headsx's image and the HeadsArgs the engine fills once at create.
struct HeadTensor {
  const char* name;
  const float* p3::HeadsArgs::*arg;
  int n0, nV;       // floats: n0 + nV * V (the head width H is 32)
  int image_rank;   // position in k_headsx's image (kernels.h heads_image_floats), -1: not in it
};
constexpr int kNumHeadTensors = 21;
extern const HeadTensor kHeadTensors[kNumHeadTensors];

// The tensors behind the fifteen outputs of P3HIP_FLAG_AUX (heads_aux.h HeadsAuxArgs), packed as fp32 in every plan and
// only under the flag: three tensor pairs no other kernel reads, whole, and of three tensors the heads read by column
// the columns kHeadTensors' kernels leave out.
struct AuxTensor {
  const char* name;
  const float* p3::HeadsAuxArgs::*arg;
  int n0, nV;       // floats of the tensor in the file: n0 + nV * V, row-major [rows][cols]
  int cols;         // 0: packed whole; else the tensor's column count, and
  int ntake;        // the columns packed, in this order: [rows][ntake]
  int take[p3::kAuxGoCols];
};
constexpr int kNumAuxTensors = 10;
extern const AuxTensor kAuxTensors[kNumAuxTensors];

// A run of k_blockw: consecutive btl blocks, their weight stream and parameter table
struct BlockwRun { size_t first; int nblk; size_t stream_off, prm_off; };

// What build_plan leaves for the engine: the path and arena offsets
struct Plan {
  PlanChoice choice;
  std::vector<BlockPlan> blocks;
  size_t init_w_off = 0; int init_nms = 0;   // the init conv: an fp16 stream, or pack_conv_f32's image (F32Conv, TfmF32)
  size_t game_w_off = 0, game_b_off = 0;
  size_t rope_cos_off = 0, rope_sin_off = 0;   // transformer
  int n_q = 0;   // INT8 paths: quantized tensors (activation scales)
  std::vector<BlockwRun> bw_runs;
  size_t heads_w_off = 0; int heads_nms = 0;   // the three head convs C -> 96, as the init conv
  size_t heads_conv_a_off = 0, heads_image_off = 0;
  FoldedBN heads_gbn{};                     // policy.gpool_bn
  size_t head_tensor_off[kNumHeadTensors] = {};   // by kHeadTensors index
  size_t aux_tensor_off[kNumAuxTensors] = {};     // by kAuxTensors index (P3HIP_FLAG_AUX only)
};

// Packs the weights of `wf` for the path choose_plan picks into `ar` and fills `plan`.  The order of Arena::add calls is
// part of the behaviour: joined launches rely on streams lying back to back.
bool build_plan(const WeightFile& wf, uint32_t flags, const Options& opt, Plan& plan, Arena& ar, std::string& err);

void spiral_rope_table(int D, double* cos_out, double* sin_out);

}  // namespace eng
