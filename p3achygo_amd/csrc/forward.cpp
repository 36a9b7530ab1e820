// forward.cpp — the forward pass of an engine: the launch arguments of the block kernels, the one launcher of a layer
// conv, one enqueue function per block family, symmetry expand / reduce, and the captured graph.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "block_i8.h"
#include "conv_any.h"
#include "conv_f32.h"
#include "conv_split.h"
#include "conv_wino.h"
#include "edge_split.h"
#include "engine.h"
#include "lconv_conv3.h"
#include "lconv_i8.h"
#include "transformer.h"
#include "transformer_f32.h"
#include "transformer_split.h"

namespace eng {
namespace {

int grid_for(const p3hip_engine* e, int npos, int npos_per_wg) {
  int wgs = (npos + npos_per_wg - 1) / npos_per_wg;
  return wgs < e->n_cu ? wgs : e->n_cu;
}

// ---- k_block launch arguments -----------------------------------------------------

// What every k_block launch that starts at fused block `first` has: the buffers and the stream's start.  The streams of
// consecutive fused blocks lie back to back in the arena (plan.cpp lay_out_runs), the fused broadcast convs' right
// before the run's first and right after its last block.
p3::BlockArgs launch_base(const p3hip_engine* e, size_t first, int npos) {
  const BlockPlan& fb = e->plan.blocks[first];
  p3::BlockArgs a{};
  a.x = e->d_x;
  a.t = e->d_s ? e->d_s : e->d_t;
  a.npos = npos;
  a.head = fb.head_of >= 0;
  a.wstream = e->d_arena + fb.stream_off - (a.head ? fb.head_bytes : 0);
  return a;
}

// Adds the fused blocks [first, first + count) to `a` as its run `r`: their BN pointers from a.blk[k] on, the run's
// macro-steps (head and tail streams included), and the pointers of the tail the broadcast block behind the run fused
// in, if any.  Returns k behind the run.
int add_run(const p3hip_engine* e, p3::BlockArgs& a, int r, size_t first, int count, int k) {
  const std::vector<BlockPlan>& blocks = e->plan.blocks;
  const BlockPlan& fb = blocks[first];
  const BlockPlan& lb = blocks[first + count - 1];
  const size_t ms_bytes = (size_t)p3::block_macro_step_bytes(e->wf.C, e->opt.c128_wg8);
  if (fb.head_of >= 0) a.nms_total += (int)(fb.head_bytes / ms_bytes);
  for (int b = 0; b < count; ++b, ++k) {
    const BlockPlan& bp = blocks[first + b];
    a.nms_total += (int)(bp.stream_bytes / ms_bytes);
    for (int j = 0; j < p3::kMaxBlockLayers; ++j) {
      a.blk[k].scale[j] = e->dev<float>(bp.bn[j].scale_off);
      a.blk[k].shift[j] = e->dev<float>(bp.bn[j].shift_off);
    }
  }
  if (lb.tail_of >= 0) {
    const BlockPlan& bb = blocks[lb.tail_of];
    a.nms_total += (int)(lb.tail_bytes / ms_bytes);
    a.tail_scale[r] = e->dev<float>(bb.bn[0].scale_off);
    a.tail_shift[r] = e->dev<float>(bb.bn[0].shift_off);
    if (bb.dense_fused) {
      a.dense_bias[r] = e->dev<float>(bb.dense_bias_off);
      a.dense_scale[r] = e->dev<float>(bb.bn[1].scale_off);
      a.dense_shift[r] = e->dev<float>(bb.bn[1].shift_off);
    }
  }
  return k;
}

// The launch's stagger and wave priorities.  `bcast`: a broadcast conv rides in the launch.
void set_schedule(const p3hip_engine* e, p3::BlockArgs& a, int npos, bool bcast) {
  // Workgroups run their positions in lockstep, so the HBM-bound phases of a launch (the fused
  // broadcast convs above all) hit the memory system from every CU at once.  A start-up stagger of
  // 10,000 cycles per step (seven steps across the CU slots of an XCD) measured -2 % on the forward
  // pass at four positions per workgroup (gpurun_out/stagger_ab.log); it costs its own length once
  // per launch, so short launches go without.  P3HIP_STAGGER overrides (0 = off).
  const bool long_launch = npos >= 3 * e->n_cu * (e->wf.C == 256 || e->opt.c128_wg8 ? 1 : 2);
  // (engines sharing the GPU with others: the spread costs its own length and another stream's kernels fill a
  // launch's tail anyway — 0.3-0.6 % of the self-play rate, gpurun_out/stagger_selfplay.log)
  const bool shared = (e->flags & P3HIP_FLAG_SHARED_DEVICE) != 0;
  a.stagger = e->opt.stagger >= 0 ? e->opt.stagger : (bcast && long_launch && !shared ? 10000 : 0);
  // two 4-wave workgroups per CU and at least two positions each: they take turns at the higher wave
  // priority (kernels.h; b12c128btl3 forward -3.5 %, b8c128nbt -2.5 % at 1024 positions, nothing at 512 and
  // below; profiles/r02_c128_pair_turns.txt).  P3HIP_NO_PAIR_TURNS=1 leaves the priorities alone.
  a.pair_turns = e->opt.pair_turns && e->wf.C == 128 && !e->opt.c128_wg8 && npos >= 4 * e->n_cu;
}

// Arguments of one k_block launch over the consecutive fused blocks [first, first + count).
p3::BlockArgs block_args(const p3hip_engine* e, size_t first, int count, int npos) {
  p3::BlockArgs a = launch_base(e, first, npos);
  a.nblk = count;
  a.nruns = 1;
  add_run(e, a, 0, first, count, 0);
  if (a.head) a.zin = a.zin2 = e->d_u;
  const int tail_of = e->plan.blocks[first + count - 1].tail_of;
  if (tail_of >= 0) {
    a.tail = 1;
    a.tout = e->d_t;
    if (e->plan.blocks[tail_of].dense_fused) {
      a.tail_dense = 1;
      a.uout = a.uout2 = e->d_u;
    }
  }
  set_schedule(e, a, npos, a.head || a.tail);
  return a;
}

// Joined launch (C = 256 btl): the runs of fused blocks from `first` on, with the broadcast blocks between them inside
// ONE k_block launch — possible when every such broadcast block has both its 1x1 convs AND its dense fused into the
// neighbouring runs (then their streams lie back to back in the arena, plan.cpp lay_out_runs).  Returns the number of
// plan blocks covered (0: not joinable) and fills `a`.
int joined_launch(const p3hip_engine* e, size_t first, int npos, p3::BlockArgs* out) {
  if (!e->opt.join) return 0;
  const std::vector<BlockPlan>& blocks = e->plan.blocks;
  std::vector<std::pair<size_t, int>> runs;   // (first block, count)
  size_t bi = first;
  int nb = 0;
  while (bi < blocks.size() && (int)runs.size() < p3::kMaxRuns) {
    const int kind = blocks[bi].kind;
    if (kind != 0) break;
    int n = 1;
    while (bi + n < blocks.size() && blocks[bi + n].kind == kind) ++n;
    if (n > p3::kMaxFuse || nb + n > p3::kMaxLaunchBlocks) break;
    runs.emplace_back(bi, n);
    nb += n;
    bi += n;
    // a broadcast block with everything fused, followed by another run?
    if (bi + 1 < blocks.size() && blocks[bi].kind == 3 && blocks[bi].first_fused && blocks[bi].last_fused &&
        blocks[bi].dense_fused && blocks[bi + 1].kind == 0) ++bi;
    else break;
  }
  if (runs.size() < 2) return 0;
  // every run's streams must lie back to back: [head r][blocks r][tail r][head r+1] ...
  for (size_t r = 0; r + 1 < runs.size(); ++r) {
    const BlockPlan& lb = blocks[runs[r].first + runs[r].second - 1];
    const BlockPlan& nf = blocks[runs[r + 1].first];
    if (lb.stream_off + lb.stream_bytes + lb.tail_bytes + nf.head_bytes != nf.stream_off) return 0;
  }
  // the loop may have stepped over a broadcast block without taking the run behind it (kMaxRuns, block limit)
  const size_t last_run_end = runs.back().first + runs.back().second;
  p3::BlockArgs a = launch_base(e, first, npos);
  a.nblk = runs[0].second;
  a.nruns = (int)runs.size();
  a.tail = blocks[last_run_end - 1].tail_of >= 0;   // the last run has a tail too when a broadcast block follows it
  a.tail_dense = 1;
  a.tout = e->d_t;
  // u alternates between two buffers inside the launch (t's buffer is free: the dense is fused) when the launch
  // neither starts with a head fed from outside nor ends with a tail read from outside; otherwise one buffer
  const bool closed = !a.head && !a.tail;
  _Float16* other = closed ? e->d_t : e->d_u;
  a.zin2 = e->d_u;   // head of an even run: what the odd run before it wrote
  a.uout = other;    // tail of an even run
  a.zin = other;     // head of an odd run
  a.uout2 = e->d_u;  // tail of an odd run
  int k = 0;
  for (size_t r = 0; r < runs.size(); ++r) {
    a.run_nblk[r] = runs[r].second;
    k = add_run(e, a, (int)r, runs[r].first, runs[r].second, k);
  }
  set_schedule(e, a, npos, true);
  *out = a;
  return (int)(last_run_end - first);
}

// Number of blocks the launch starting at block `first` covers: consecutive blocks of the fused
// kernel's kind, at most kMaxFuse (1 when P3HIP_NO_FUSE is set: one launch per block).
int fused_run(const p3hip_engine* e, size_t first) {
  const std::vector<BlockPlan>& blocks = e->plan.blocks;
  const int kind = blocks[first].kind;
  if (kind != 0 && kind != 1) return 0;
  int n = 1;
  while (e->opt.fuse && n < p3::kMaxFuse && first + n < blocks.size() && blocks[first + n].kind == kind) ++n;
  return n;
}

}  // namespace
}  // namespace eng

// k_blockw: the code object assembled from csrc/asm/blockw_gen.py's output rides in the library as a blob
// (blockw_blob.S); one module per engine (modules are per device).  Kernel arguments: csrc/asm/blockw_gen.py.
extern "C" const unsigned char p3_blockw_hsaco[];
extern "C" const unsigned char p3_blockw_hsaco_end[];

namespace eng {
namespace {

struct BlockwArgs {
  const void* x; const void* ws; const void* prm;
  int npos, nblk, nwg, pad;
  void* stamps;
  unsigned long long pad2[2];
};
static_assert(sizeof(BlockwArgs) == 64, "kernarg layout of k_blockw");

bool load_blockw(p3hip_engine* e) {
  if (e->bw_fn) return true;
  if (!e->check(hipModuleLoadData(&e->bw_mod, p3_blockw_hsaco), "hipModuleLoadData k_blockw")) return false;
  const std::string name = "k_blockw_L" + std::to_string(e->wf.inner) + (e->opt.blockw_diag ? "_diag" : "");
  if (!e->check(hipModuleGetFunction(&e->bw_fn, e->bw_mod, name.c_str()), "hipModuleGetFunction k_blockw")) return false;
  if (e->opt.blockw_diag) {
    constexpr size_t bytes = 8 * 16 * 4 * 24 * 8;   // [workgroup 0..7][block][wave][stamp]
    if (!e->check(hipMalloc((void**)&e->d_bw_stamps, bytes), "hipMalloc stamps") ||
        !e->check(hipMemsetAsync(e->d_bw_stamps, 0, bytes, e->stream), "hipMemset stamps")) return false;
  }
  return true;
}

bool launch_blockw(p3hip_engine* e, const BlockwRun& run, int npos) {
  if (!load_blockw(e)) return false;
  BlockwArgs a{};
  a.x = e->d_x;
  a.ws = e->d_arena + run.stream_off;
  a.prm = e->d_arena + run.prm_off;
  a.npos = npos;
  a.nblk = run.nblk;
  a.nwg = npos < e->n_cu ? npos : e->n_cu;
  a.stamps = e->d_bw_stamps;
  size_t size = sizeof a;
  void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  return e->check(hipModuleLaunchKernel(e->bw_fn, a.nwg, 1, 1, 256, 1, 1, 0, e->stream, nullptr, cfg), "launch k_blockw");
}

// Enqueues `launch`; `timed` (p3hip_time_trunk_kernel, null otherwise) counts the launches put between an event pair of
// e->blk_ev, while events last.
template <class Launch>
bool timed_launch(p3hip_engine* e, int* timed, Launch&& launch) {
  const bool on = timed && 2 * *timed + 1 < (int)e->blk_ev.size();
  if (on) hipEventRecord(e->blk_ev[2 * *timed], e->stream);
  if (!launch()) return false;
  if (on) hipEventRecord(e->blk_ev[2 * (*timed)++ + 1], e->stream);
  return true;
}

// ---- the enqueue functions: stem, one per block family, heads ---------------------------------------

// a 1x1 conv of the k_conv1x1 family: 0 conv_first, 1 conv_last of a broadcast block, 2 the head convs
hipError_t launch_conv1x1(const p3hip_engine* e, int which, const p3::Conv1x1Args& a) {
  return runs_conv_any(e->plan.choice) ? p3::launch_conv1x1_any(e->wf.C, which, a, e->n_cu, e->stream)
                                    : p3::launch_conv1x1(e->wf.C, which, a, e->n_cu, e->stream);
}

bool enqueue_stem(p3hip_engine* e, const Pass& p) {
  const Plan& pl = e->plan;
  const int C = e->wf.C;
  if (is_f32(e->trunk_path())) {
    const p3::InitF32Args a{p.feats, (float*)e->d_x, p.npos, C, e->dev<float>(pl.init_w_off), e->dev<float>(pl.game_w_off),
                            e->dev<float>(pl.game_b_off)};
    return e->check(p3::launch_init_f32(a, e->n_cu, e->stream), "launch k_init_f32");
  }
  p3::InitArgs a{};
  a.feats = p.feats; a.x = e->d_x; a.npos = p.npos;
  a.wstream = e->d_arena + pl.init_w_off; a.nms_total = pl.init_nms;
  a.game_w = e->dev<float>(pl.game_w_off); a.game_b = e->dev<float>(pl.game_b_off);
  // the low-latency plans: a position's output passes on as many workgroups, where the launch's split says so
  if (e->trunk_path() == Path::Split || e->trunk_path() == Path::TfmSplit) {
    int stem = 1, dense = 1, heads = 1;
    edge_split_of(e, p.npos, &stem, &dense, &heads);
    if (stem > 1) return e->check(p3::launch_init_split(C, a, stem, e->n_cu, e->stream), "launch k_init_split");
  }
  return e->check(runs_conv_any(e->plan.choice) ? p3::launch_init_any(C, a, grid_for(e, p.npos, 1), e->stream)
                                             : p3::launch_init(C, a, grid_for(e, p.npos, 1), e->stream), "launch k_init");
}

bool enqueue_tfm_block(p3hip_engine* e, const Pass& p, const BlockPlan& bp) {
  const int d = e->wf.model_C, D = e->plan.choice.tfm_D, npos = p.npos;
  hipStream_t s = e->stream;
  const size_t per = (size_t)e->rows * p3::kTfmLPad * d;   // one of q, k, v: [rows][head][384][D]
  _Float16 *q = e->d_qkv, *k = q + per, *v = k + per, *o = e->d_t;
  p3::TfmQkvArgs a{e->d_x, q, k, v, npos, e->dev<float>(bp.tfm.rms_in), e->d_arena + bp.tfm.wqkv,
                   e->dev<float>(e->plan.rope_cos_off), e->dev<float>(e->plan.rope_sin_off)};
  // (TfmSplit: the split of this launch; (1, 64) is the default plan's launches, which launch_tfm_*_split then call)
  int parts = 1, tokens = 64;
  if (e->trunk_path() == Path::TfmSplit) tfm_split_of(e, npos, &parts, &tokens);
  if (!e->check(p3::launch_tfm_qkv_split(d, D, a, tokens, s), "launch k_tfm_qkv")) return false;
  const p3::TfmAttnArgs b{q, k, v, o, npos, e->plan.choice.tfm_heads};
  if (!timed_launch(e, p.timed, [&] { return e->check(p3::launch_tfm_attn_split(D, b, parts, s), "launch k_tfm_attn"); }))
    return false;
  const p3::TfmFfnArgs f{o, e->d_x, npos, e->d_arena + bp.tfm.wo, e->dev<float>(bp.tfm.rms_out),
                         e->d_arena + bp.tfm.wgu, e->d_arena + bp.tfm.wdown};
  return e->check(p3::launch_tfm_ffn_split(d, f, tokens, s), "launch k_tfm_ffn");
}

bool enqueue_tfm_block_f32(p3hip_engine* e, const Pass& p, const BlockPlan& bp) {
  const int d = e->wf.model_C, D = e->plan.choice.tfm_D, npos = p.npos;
  hipStream_t s = e->stream;
  const size_t per = (size_t)e->rows * p3::kTfmLPad * d;   // one of q, k, v: [rows][head][384][D] floats
  float *x = (float*)e->d_x, *q = (float*)e->d_qkv, *k = q + per, *v = k + per, *o = (float*)e->d_t;
  const p3::TfmQkvF32Args a{x, q, k, v, npos, d, D, e->dev<float>(bp.tfm.rms_in), e->dev<float>(bp.tfm.wqkv),
                            e->dev<float>(e->plan.rope_cos_off), e->dev<float>(e->plan.rope_sin_off)};
  if (!e->check(p3::launch_tfm_qkv_f32(a, s), "launch k_tfm_qkv_f32")) return false;
  const p3::TfmAttnF32Args b{q, k, v, o, npos, e->plan.choice.tfm_heads};
  if (!timed_launch(e, p.timed, [&] { return e->check(p3::launch_tfm_attn_f32(D, b, s), "launch k_tfm_attn_f32"); }))
    return false;
  const p3::TfmFfnF32Args f{o, x, npos, d, e->dev<float>(bp.tfm.wo), e->dev<float>(bp.tfm.rms_out),
                            e->dev<float>(bp.tfm.wgu), e->dev<float>(bp.tfm.wdown)};
  return e->check(p3::launch_tfm_ffn_f32(f, s), "launch k_tfm_ffn_f32");
}

// The regions of a layer-wise block (LayerPlan) in buffers of element type T
template <class T>
struct Regions {
  T* buf[5];
  explicit Regions(const p3hip_engine* e) {
    const size_t half = (size_t)e->rows * e->wf.Cb * kNLoc;   // elements of one C_b-channel tensor
    T *x = (T*)e->d_x, *t = (T*)e->d_t, *u = (T*)e->d_u;
    buf[0] = x; buf[1] = t; buf[2] = t + half; buf[3] = u; buf[4] = u + half;
  }
};

// the fields p3::LConvArgs, p3::LConvI8Args and p3::LConvF32Args share
template <class Args, class T>
void fill_layer(const p3hip_engine* e, Args& a, const LayerPlan& lp, const Regions<T>& r, int npos) {
  a.in = r.buf[lp.in_buf]; a.out = r.buf[lp.out_buf]; a.npos = npos;
  a.out2 = lp.out2_buf >= 0 ? reinterpret_cast<decltype(a.out2)>(r.buf[lp.out2_buf]) : nullptr;
  a.pre = lp.pre; a.act = lp.act; a.res = lp.res; a.dual = lp.dual;
  if (a.pre) { a.scale_in = e->dev<float>(lp.pre_bn.scale_off); a.shift_in = e->dev<float>(lp.pre_bn.shift_off); }
  if (a.act == 1 || a.dual) { a.scale_out = e->dev<float>(lp.out_bn.scale_off); a.shift_out = e->dev<float>(lp.out_bn.shift_off); }
}

// The conv of one LayerPlan through the kernel the engine's state selects (layer_kernel).  `what`: the name e->check
// reports a failed launch under, the kernel's own by default
bool launch_layer(p3hip_engine* e, const Pass& p, const LayerPlan& lp, const char* what = nullptr) {
  const LayerKernel k = layer_kernel(e, lp.kw);
  const bool conv3 = e->trunk_path() == Path::Int8Conv3;
  switch (k) {
    case LayerKernel::LconvF32: {
      p3::LConvF32Args a{};
      fill_layer(e, a, lp, Regions<float>(e), p.npos);
      a.cin = lp.cin; a.cout = lp.cout; a.w = e->dev<float>(lp.w_off);
      return e->check(p3::launch_lconv_f32(lp.kw, a, e->n_cu, e->stream), what ? what : "launch k_lconv_f32");
    }
    case LayerKernel::Sconv: {
      p3::SConvArgs a{};
      fill_layer(e, a, lp, Regions<_Float16>(e), p.npos);
      a.cin = lp.cin; a.cout = lp.cout; a.w = e->d_arena + lp.w_off;
      // the split: P3HIP_SPLIT's, or the launch's own choice
      if (e->opt.split_s) { a.strips = e->opt.split_s; a.tile = e->opt.split_t; }
      else p3::sconv_split(a.npos, lp.kw, a.cout, e->n_cu, &a.strips, &a.tile);
      return e->check(p3::launch_sconv(lp.kw, a, e->n_cu, e->stream), what ? what : "launch k_sconv");
    }
    case LayerKernel::Wconv: {
      p3::WConvArgs a{};
      fill_layer(e, a, lp, Regions<_Float16>(e), p.npos);
      a.cin = lp.cin; a.cout = lp.cout; a.w = e->d_arena + lp.wino_off;
      return e->check(p3::launch_wconv(a, e->n_cu, e->stream), what ? what : "launch k_wconv");
    }
    case LayerKernel::LconvI8:
    case LayerKernel::LconvI8Any: {
      // (the callers check int8_ready) the fp16 plan's regions, an int8 tensor where that stores an activated one
      p3::LConvI8Args a{};
      fill_layer(e, a, lp, Regions<_Float16>(e), p.npos);
      a.w = e->dev<int8_t>(lp.q_off); a.w_scale = e->dev<float>(lp.qs_off);
      a.act_scale = e->d_ascale; a.in_scale = lp.qidx; a.out_scale = lp.qidx + 1;
      // Int8Conv3: the consumer of the last 3x3's activated output is the fp16 1x1 expand
      if (conv3 && lp.out_qidx < 0)
        return e->check(p3::launch_lconv_i8_f16(k == LayerKernel::LconvI8Any, lp.kw, lp.cin, lp.cout, a, e->stream),
                        what ? what : "launch k_lconv_i8_f16");
      return k == LayerKernel::LconvI8Any
                 ? e->check(p3::launch_lconv_i8_any(lp.kw, lp.cin, lp.cout, a, e->stream), what ? what : "launch k_lconv_i8_any")
                 : e->check(p3::launch_lconv_i8(lp.kw, lp.cin, lp.cout, a, e->stream), what ? what : "launch k_lconv_i8");
    }
    case LayerKernel::Lconv:
    case LayerKernel::LconvAny: {
      p3::LConvArgs a{};
      fill_layer(e, a, lp, Regions<_Float16>(e), p.npos);
      a.wstream = e->d_arena + lp.w_off; a.nms_total = lp.nms;
      // Int8Conv3: the consumer of the 1x1 reduce's activated output is the first int8 3x3 (calibration: the fp16 plan)
      if (conv3 && lp.out_qidx >= 0 && !e->calibrating)
        return e->check(p3::launch_lconv_q8(k == LayerKernel::LconvAny, lp.kw, lp.cin, lp.cout, a, e->d_ascale, lp.out_qidx,
                                            e->n_cu, e->stream), what ? what : "launch k_lconv_q8");
      return k == LayerKernel::LconvAny
                 ? e->check(p3::launch_lconv_any(lp.kw, lp.cin, lp.cout, a, e->n_cu, e->stream), what ? what : "launch k_lconv_any")
                 : e->check(p3::launch_lconv(lp.kw, lp.cin, lp.cout, a, e->n_cu, e->stream), what ? what : "launch k_lconv");
    }
  }
  return false;
}

// A layer-wise block on every path but the fused INT8 ones' runs (enqueue_block_i8); the calibration runs of the INT8
// paths are the fp16 plan + absmax
bool enqueue_layerwise_block(p3hip_engine* e, const Pass& p, const BlockPlan& bp) {
  for (const LayerPlan& lp : bp.layers) {
    if (e->calibrating && lp.qidx >= 0) {
      // MinMax calibration: the absmax of this conv's quantized input, the activated tensor (pre: mish(bn0(x)),
      // which the fp16 plan never stores) folded into the running maximum
      p3::AbsmaxArgs m{};
      m.in = Regions<_Float16>(e).buf[lp.in_buf]; m.npos = p.npos; m.C = lp.cin; m.amax = e->d_amax + lp.qidx;
      if (lp.pre) { m.scale = e->dev<float>(lp.pre_bn.scale_off); m.shift = e->dev<float>(lp.pre_bn.shift_off); }
      if (!e->check(p3::launch_absmax(m, e->n_cu, e->stream), "launch k_absmax")) return false;
    }
    if (!timed_launch(e, lp.kw == 3 ? p.timed : nullptr, [&] { return launch_layer(e, p, lp); })) return false;
  }
  return true;
}

p3::BDenseArgs bdense_args(const p3hip_engine* e, const BlockPlan& bp, int npos) {
  p3::BDenseArgs d{};
  d.t = e->d_t; d.u = e->d_u; d.npos = npos;
  d.wstream = e->d_arena + bp.dense_off; d.nms_total = bp.dense_nms;
  d.bias = e->dev<float>(bp.dense_bias_off);
  d.scale = e->dev<float>(bp.bn[1].scale_off); d.shift = e->dev<float>(bp.bn[1].shift_off);
  return d;
}

// A broadcast block of F32Conv and Split: conv_first and conv_last, the block's two layers, through the path's layer
// kernel; between them the dense in fp32, or (Split) as ConvAny's
bool enqueue_broadcast_block_layers(p3hip_engine* e, const Pass& p, const BlockPlan& bp) {
  const int C = e->wf.C, npos = p.npos;
  const bool f32 = e->trunk_path() == Path::F32Conv;
  if (!launch_layer(e, p, bp.layers[0], f32 ? "launch conv_first (fp32)" : "launch conv_first (k_sconv)")) return false;
  if (f32) {
    const p3::BDenseF32Args d{(float*)e->d_t, (float*)e->d_u, npos, C, e->dev<float>(bp.dense_off), e->dev<float>(bp.dense_bias_off),
                              e->dev<float>(bp.bn[1].scale_off), e->dev<float>(bp.bn[1].shift_off)};
    if (!e->check(p3::launch_bdense_f32(d, e->n_cu, e->stream), "launch k_bdense_f32")) return false;
  } else {
    int stem = 1, dense = 1, heads = 1;
    edge_split_of(e, npos, &stem, &dense, &heads);
    const p3::BDenseArgs d = bdense_args(e, bp, npos);
    if (!(dense > 1 ? e->check(p3::launch_bdense_split(C, d, dense, e->n_cu, e->stream), "launch k_bdense_split")
                    : e->check(p3::launch_bdense_any(C, d, grid_for(e, npos, 1), e->stream), "launch bdense")))
      return false;
  }
  return launch_layer(e, p, bp.layers[1], f32 ? "launch conv_last (fp32)" : "launch conv_last (k_sconv)");
}

// A broadcast block in fp16: whatever of conv_first, dense and conv_last the neighbouring block launches did not take
bool enqueue_broadcast_block(p3hip_engine* e, const Pass& p, const BlockPlan& bp) {
  const int C = e->wf.C, npos = p.npos;
  const LayerPlan &first = bp.layers[0], &last = bp.layers[1];
  p3::Conv1x1Args c0{};
  c0.in = e->d_x; c0.out16 = e->d_t; c0.npos = npos;
  c0.wstream = e->d_arena + first.w_off; c0.nms_total = first.nms;
  c0.scale = e->dev<float>(bp.bn[0].scale_off); c0.shift = e->dev<float>(bp.bn[0].shift_off);
  if (!bp.first_fused && !e->check(launch_conv1x1(e, 0, c0), "launch conv_first")) return false;
  const p3::BDenseArgs d = bdense_args(e, bp, npos);
  if (!(bp.first_fused && bp.dense_fused) &&
      !e->check(runs_conv_any(e->plan.choice) ? p3::launch_bdense_any(C, d, grid_for(e, npos, 1), e->stream)
                                           : p3::launch_bdense(C, d, grid_for(e, npos, 1), e->stream), "launch bdense")) return false;
  p3::Conv1x1Args c1{};
  c1.in = e->d_u; c1.out16 = e->d_x; c1.npos = npos;
  c1.wstream = e->d_arena + last.w_off; c1.nms_total = last.nms;
  return bp.last_fused || e->check(launch_conv1x1(e, 1, c1), "launch conv_last");
}

// Int8Fused256 / Int8Fused128: one launch runs the block's convs with the activations in LDS; the layers carry its tensors
bool enqueue_block_i8(p3hip_engine* e, const Pass& p, const BlockPlan& bp) {
  p3::BlockI8Args a{};
  a.x = e->d_x; a.npos = p.npos; a.inner = e->wf.inner;
  a.act_scale = e->d_ascale; a.q0 = bp.layers[0].qidx;
  for (size_t j = 0; j < bp.layers.size(); ++j) {
    const LayerPlan& lp = bp.layers[j];
    a.w[j] = e->dev<int8_t>(lp.q_off); a.w_scale[j] = e->dev<float>(lp.qs_off);
    // bn_j is the prologue of conv 0 and the epilogue of conv j - 1
    const FoldedBN& bn = j == 0 ? lp.pre_bn : bp.layers[j - 1].out_bn;
    a.scale[j] = e->dev<float>(bn.scale_off); a.shift[j] = e->dev<float>(bn.shift_off);
  }
  auto launch = [&] { return e->check(p3::launch_block_i8(e->wf.C, a, e->n_cu, e->stream), "launch k_block_i8"); };
  return timed_launch(e, p.timed, launch);
}

// Blockw: the k_blockw run that starts at block bi; *covered: its blocks
bool enqueue_blockw_run(p3hip_engine* e, const Pass& p, size_t bi, int* covered) {
  const int r = e->plan.blocks[bi].bw_run;
  if (r < 0) { e->err = "internal error: no k_blockw run starts at this block"; return false; }
  const BlockwRun& run = e->plan.bw_runs[r];
  *covered = run.nblk;
  return timed_launch(e, p.timed, [&] { return launch_blockw(e, run, p.npos); });
}

// Fused: one k_block launch over the run that starts at block bi, or over several runs (joined_launch); *covered: the
// plan blocks it took
bool enqueue_fused_run(p3hip_engine* e, const Pass& p, size_t bi, int* covered) {
  p3::BlockArgs a;
  *covered = joined_launch(e, bi, p.npos, &a);
  if (*covered == 0) {
    *covered = fused_run(e, bi);
    a = block_args(e, bi, *covered, p.npos);
  }
#ifdef P3_DIAG
  {
    static const int which = getenv("P3DIAG_LAUNCH") ? atoi(getenv("P3DIAG_LAUNCH")) : 1;
    constexpr size_t bytes = (size_t)p3::kStampWgs * 8 * p3::kStampSections * p3::kStampSlots * 8;
    if (!e->d_stamps && hipMalloc((void**)&e->d_stamps, bytes) == hipSuccess) hipMemset(e->d_stamps, 0, bytes);
    constexpr size_t span_bytes = (size_t)p3::kSpanWgs * p3::kSpanSlots * 8;
    if (!e->d_spans && hipMalloc((void**)&e->d_spans, span_bytes) == hipSuccess) hipMemset(e->d_spans, 0, span_bytes);
    // joined launches: ONE block launch per forward pass (index 0); P3DIAG_RUN picks the run whose phases are stamped
    static const int which_run = getenv("P3DIAG_RUN") ? atoi(getenv("P3DIAG_RUN")) : 1;
    const int idx = (a.nruns > 1) ? 0 : which;
    a.stamp_run = (a.nruns > 1) ? which_run : 0;
    a.spans = (e->launch_index == idx) ? e->d_spans : nullptr;
    a.stamps = (e->launch_index++ == idx) ? e->d_stamps : nullptr;
  }
#endif
  const int kind = e->plan.blocks[bi].kind;
  auto launch = [&] {
    return e->check(p3::launch_block(e->wf.C, kind, e->wf.inner, e->opt.c128_wg8, a, e->n_cu, e->stream), "launch k_block");
  };
  return timed_launch(e, p.timed, launch);
}

bool enqueue_heads(p3hip_engine* e, const Pass& p) {
  const int C = e->wf.C;
  if (is_f32(e->trunk_path())) {
    p3::LConvF32Args hc{};   // the three head convs C -> 96 in fp32, hp in k_heads' layout
    hc.in = (const float*)e->d_x; hc.out = e->d_hp; hc.npos = p.npos; hc.cin = C; hc.cout = 128; hc.hp = 1;
    hc.w = e->dev<float>(e->plan.heads_w_off);
    if (!e->check(p3::launch_lconv_f32(1, hc, e->n_cu, e->stream), "launch head convs (fp32)")) return false;
  } else if (!e->plan.choice.heads_fused) {
    p3::Conv1x1Args c{};
    c.in = e->d_x; c.out32 = e->d_hp; c.npos = p.npos;
    c.wstream = e->d_arena + e->plan.heads_w_off; c.nms_total = e->plan.heads_nms;
    if (!e->check(launch_conv1x1(e, 2, c), "launch head convs")) return false;
  }
  const bool aux = (e->flags & P3HIP_FLAG_AUX) != 0;
  if (aux && e->plan.choice.heads_fused) {
    // k_headsx keeps the head convs' output to itself: the launch the unfused path makes, for k_heads_aux alone
    p3::Conv1x1Args c{};
    c.in = e->d_x; c.out32 = e->d_hp; c.npos = p.npos;
    c.wstream = e->d_arena + e->plan.heads_w_off; c.nms_total = e->plan.heads_nms;
    if (!e->check(launch_conv1x1(e, 2, c), "launch head convs (aux)")) return false;
  }
  p3::HeadsArgs h = e->heads_args;   // the weight pointers never change after create
  h.x = e->d_x; h.hp = e->d_hp; h.out = p.out; h.res = p.res; h.npos = p.npos;
  // the low-latency plans: k_heads in three launches over more workgroups, where the launch's split says so (k_headsx
  // stays whole: edge_split.h)
  int hparts = 1;
  if (!e->plan.choice.heads_fused && (e->trunk_path() == Path::Split || e->trunk_path() == Path::TfmSplit)) {
    int stem = 1, dense = 1;
    edge_split_of(e, p.npos, &stem, &dense, &hparts);
  }
  if (!(e->plan.choice.heads_fused ? e->check(p3::launch_headsx(C, h, e->n_cu, e->stream), "launch k_headsx")
        : hparts > 1               ? e->check(p3::launch_heads_split(h, e->d_pool, hparts, e->stream), "launch k_heads_pool / points / softmax")
                                   : e->check(p3::launch_heads(h, p.npos, e->stream), "launch k_heads"))) return false;
  if (!aux) return true;
  p3::HeadsAuxArgs x = e->aux_args;
  x.hp = e->d_hp; x.aux = e->d_aux; x.npos = p.npos;
  return e->check(p3::launch_heads_aux(x, e->n_cu, e->stream), "launch k_heads_aux");
}

}  // namespace

// The split of a TfmSplit engine's launches over npos positions: P3HIP_TFM_SPLIT's, or the chooser's
void tfm_split_of(const p3hip_engine* e, int npos, int* parts, int* tokens) {
  if (e->opt.tfm_split_s) { *parts = e->opt.tfm_split_s; *tokens = e->opt.tfm_split_t; }
  else p3::tfm_split(npos, e->plan.choice.tfm_heads, e->n_cu, parts, tokens);
}

// The parts of a low-latency engine's stem, broadcast dense and heads launches over npos positions: P3HIP_EDGE_SPLIT's, or
// the chooser's
void edge_split_of(const p3hip_engine* e, int npos, int* stem, int* dense, int* heads) {
  if (e->opt.edge_s) { *stem = e->opt.edge_s; *dense = e->opt.edge_d; *heads = e->opt.edge_h; }
  else p3::edge_split(npos, e->wf.C, e->n_cu, stem, dense, heads);
}

// The kernel of the layer convs: the path's, and on the INT8 paths while they calibrate the fp16 plan's.  (The fused INT8
// paths run whole blocks, enqueue_block_i8, once calibrated; Int8Fused128 calibrates through the runtime-width kernel:
// k_lconv has no C = 128 / C_b = 64 instantiations)
// Int8Conv3 decides per layer: a 3x3 conv the INT8 kernel, a 1x1 conv (and every conv while calibrating) the fp16 kernel,
// templated or runtime-width as the trunk's fp16 plan
LayerKernel layer_kernel(const p3hip_engine* e, int kw) {
  const Path path = e->trunk_path();
  if (path == Path::Int8Conv3) {
    const bool any = e->plan.choice.any_width;
    if (kw == 3 && !e->calibrating) return any ? LayerKernel::LconvI8Any : LayerKernel::LconvI8;
    return any ? LayerKernel::LconvAny : LayerKernel::Lconv;
  }
  // Winograd3: a 3x3 conv k_wconv, a 1x1 conv the kernel of the trunk's fp16 plan
  if (path == Path::Winograd3) return kw == 3 ? LayerKernel::Wconv : e->plan.choice.any_width ? LayerKernel::LconvAny : LayerKernel::Lconv;
  if (path == Path::F32Conv) return LayerKernel::LconvF32;
  if (path == Path::Split) return LayerKernel::Sconv;
  if (is_int8(path) && !e->calibrating) return path == Path::Int8Any ? LayerKernel::LconvI8Any : LayerKernel::LconvI8;
  return runs_conv_any(e->plan.choice) || path == Path::Int8Fused128 ? LayerKernel::LconvAny : LayerKernel::Lconv;
}

const char* layer_kernel_name(LayerKernel k, int kw, int cin, int cout) {
  switch (k) {
    case LayerKernel::Lconv: return cin == 192 ? "k_lconv<3,192,192>" : "k_lconv<3,64,64>";   // (the 3x3 convs: the timed ones)
    case LayerKernel::LconvAny: return p3::lconv_any_kernel_name(kw);
    case LayerKernel::LconvI8: return p3::lconv_i8_kernel_name(kw, cin, cout);
    case LayerKernel::LconvI8Any: return p3::lconv_i8_any_kernel_name(kw);
    case LayerKernel::LconvF32: return p3::lconv_f32_kernel_name(kw);
    case LayerKernel::Sconv: return p3::sconv_kernel_name(kw);
    case LayerKernel::Wconv: return p3::wconv_kernel_name();
  }
  return nullptr;
}

// Enqueues the whole forward pass `p`: stem, blocks, heads.
bool enqueue_forward(p3hip_engine* e, const Pass& p) {
  const Path path = e->trunk_path();
  const std::vector<BlockPlan>& blocks = e->plan.blocks;
  if (!enqueue_stem(e, p)) return false;
#ifdef P3_DIAG
  e->launch_index = 0;
#endif
  // debugging aid (tools/gpu_blockw_ab.py xdiff, tests/test_trunk_blocks_gpu.py): stop the forward pass in front of
  // plan block opt.stop_block (P3HIP_DEBUG_STOP_BLOCK when the engine was created); a value equal to the block count
  // stops it after the last block, in front of the heads (which take d_t, the transformer's o, as scratch)
  const int stop_block = e->opt.stop_block;
  e->last_npos = p.npos;
  for (size_t bi = 0; bi < blocks.size(); ++bi) {
    if (stop_block >= 0 && (int)bi >= stop_block) return true;
    const BlockPlan& bp = blocks[bi];
    int covered = 1;   // plan blocks the launch(es) took
    bool ok = false;
    switch (bp.kind) {
      case 5:
        ok = path == Path::TfmF32 ? enqueue_tfm_block_f32(e, p, bp) : enqueue_tfm_block(e, p, bp);
        break;
      case 3:
        ok = path == Path::F32Conv || path == Path::Split ? enqueue_broadcast_block_layers(e, p, bp) : enqueue_broadcast_block(e, p, bp);
        break;
      case 4:
        ok = is_int8_fused(path) && !e->calibrating ? enqueue_block_i8(e, p, bp) : enqueue_layerwise_block(e, p, bp);
        break;
      default:   // 0 btl, 1 nbt
        ok = path == Path::Blockw ? enqueue_blockw_run(e, p, bi, &covered) : enqueue_fused_run(e, p, bi, &covered);
    }
    if (!ok) return false;
    bi += covered - 1;
  }
  if (stop_block == (int)blocks.size()) return true;
  return enqueue_heads(e, p);
}

// P3HIP_FLAG_SYMMETRY_SLOT: first[] and the masks of `n` dense rows into the pinned table, and its upload on the stream
bool stage_sym_table(p3hip_engine* e, const unsigned char* masks, int n) {
  const size_t B = (size_t)e->batch;
  int* first = reinterpret_cast<int*>(e->h_symtab);
  int total = 0;
  e->tab_n = e->tab_total = 0;
  if (p3::sym_rows(masks, n, e->rows, first, &total) != 0) {
    e->err = "P3HIP_FLAG_SYMMETRY_SLOT: the symmetry masks of the " + std::to_string(n) + " slots of this run add up to " +
             std::to_string(total) + " copies, the engine was created with symmetry_rows " + std::to_string(e->rows) +
             " (nothing was launched; lower masks with p3hip_set_slot_symmetries and run again)";
    return false;
  }
  memcpy(e->h_symtab + B * 4, masks, (size_t)n);
  // one copy where the two arrays are adjacent (the full static batch), else one each
  const bool ok = (size_t)n == B
      ? e->check(hipMemcpyAsync(e->d_symtab, e->h_symtab, B * 5, hipMemcpyHostToDevice, e->stream), "H2D symmetry table")
      : e->check(hipMemcpyAsync(e->d_symtab, e->h_symtab, (size_t)n * 4, hipMemcpyHostToDevice, e->stream), "H2D symmetry table") &&
        e->check(hipMemcpyAsync(e->d_symtab + B * 4, e->h_symtab + B * 4, (size_t)n, hipMemcpyHostToDevice, e->stream), "H2D symmetry masks");
  if (!ok) return false;
  e->tab_n = n;
  e->tab_total = total;
  return true;
}

int sym_rows_of(const p3hip_engine* e, int n) {
  if (n < 1 || n > e->tab_n) return -1;
  return n == e->tab_n ? e->tab_total : reinterpret_cast<const int*>(e->h_symtab)[n];
}

// k_sym_expand / k_sym_expand_slots: the `n` records at `src` -> their copies in d_feats
bool expand_sym(p3hip_engine* e, const unsigned char* src, int n) {
  if (e->sym_slot) {
    const int total = sym_rows_of(e, n);
    if (total < 0) {
      e->err = "P3HIP_FLAG_SYMMETRY_SLOT: " + std::to_string(n) + " positions asked for, the last p3hip_run / p3hip_upload staged the masks of " +
               std::to_string(e->tab_n);
      return false;
    }
    p3::SymExpandSlotsArgs x{};
    x.in = src; x.out = e->d_feats; x.first = e->tab_first(); x.mask = e->tab_mask(); x.n = n; x.cap = e->rows;
    return e->check(p3::launch_sym_expand_slots(x, total, e->stream), "launch k_sym_expand_slots");
  }
  p3::SymExpandArgs x{};
  x.in = src; x.out = e->d_feats; x.n = n; x.k = e->sym_k;
  for (int j = 0; j < p3::kNumSyms; ++j) x.syms[j] = e->sym_syms[j];
  return e->check(p3::launch_sym_expand(x, e->stream), "launch k_sym_expand");
}

namespace {

// P3HIP_FLAG_SYMMETRY_AVG: the `p.npos` slots' records in p.feats -> k copies each in d_feats -> the forward pass over
// n k rows (the heads write d_cout, never d_res) -> the averaged rows in p.out, and the result records in p.res.
// P3HIP_FLAG_SYMMETRY_SLOT: the same over the staged table's rows.
bool enqueue_sym(p3hip_engine* e, const Pass& p) {
  const int total = e->sym_slot ? sym_rows_of(e, p.npos) : p.npos * e->sym_k;
  if (!expand_sym(e, p.feats, p.npos) || !enqueue_forward(e, Pass{e->d_feats, total, e->d_cout})) return false;
  if (e->sym_slot) {
    p3::SymReduceSlotsArgs r{};
    r.rows = e->d_cout; r.out = p.out; r.res = p.res; r.first = e->tab_first(); r.mask = e->tab_mask(); r.n = p.npos; r.cap = e->rows;
    return e->check(p3::launch_sym_reduce_slots(r, total, e->stream), "launch k_sym_reduce_slots");
  }
  p3::SymReduceArgs r{};
  r.rows = e->d_cout; r.out = p.out; r.res = p.res; r.n = p.npos; r.k = e->sym_k;
  for (int j = 0; j < p3::kNumSyms; ++j) r.syms[j] = e->sym_syms[j];
  return e->check(p3::launch_sym_reduce(r, e->stream), "launch k_sym_reduce");
}

// Captures `enqueue` on the engine's stream, one linear chain, and instantiates it.  False (nothing was executed, nothing
// is left behind, HIP's error state is cleared): the capture did not come about.
template <class Enqueue>
bool capture_pass(p3hip_engine* e, Enqueue&& enqueue, hipGraph_t* graph, hipGraphExec_t* exec) {
  *graph = nullptr;
  *exec = nullptr;
  if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  const bool ok = enqueue();
  const hipError_t ce = hipStreamEndCapture(e->stream, graph);
  if (!ok || ce != hipSuccess || !*graph || hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0) != hipSuccess) {
    if (*graph) hipGraphDestroy(*graph);
    *graph = nullptr;
    *exec = nullptr;
    (void)hipGetLastError();
    return false;
  }
  return true;
}

void destroy_slot(GraphSlot& s) {
  if (s.exec) hipGraphExecDestroy(s.exec);
  if (s.graph) hipGraphDestroy(s.graph);
  s = GraphSlot{};
}

// The pass of a P3HIP_FLAG_LAUNCH_GRAPH_ANY engine: the table says whether its key is launched, captured or replayed.
// e->last_npos: the forward rows, set by run_pass.
template <class Enqueue>
bool run_pass_any(p3hip_engine* e, const Pass& p, Enqueue&& enqueue) {
  // calibration passes run other kernels (the fp16 plan + absmax), a stopped engine is a debugging aid, and a pass
  // without rows (P3HIP_FLAG_SYMMETRY_SLOT: more slots than the staged table) only fetches its error
  // P3HIP_GRAPH_MAX_ROWS: a partial pass of more forward rows is not worth a graph
  const bool too_long = e->opt.graph_max_rows > 0 && p.npos != e->batch && e->last_npos > e->opt.graph_max_rows;
  if (e->graph_failed || e->calibrating || e->opt.stop_block >= 0 || e->last_npos < 1 || too_long) {
    e->graph_table.count_launch();
    return enqueue();
  }
  const gt::Step step = e->graph_table.see(gt::Key{p.npos, e->last_npos, p.feats, p.res}, e->graph_seq++);
  if (step.action == gt::kLaunch) return enqueue();
  GraphSlot& slot = e->graph_slots[step.slot];
  if (step.action == gt::kReplay) return e->check(hipGraphLaunch(slot.exec, e->stream), "hipGraphLaunch");
  if (slot.exec) {
    // the table gave up the graph replayed longest ago for this one: nothing of it may be in flight when it goes
    if (!e->check(hipStreamSynchronize(e->stream), "sync")) return false;
    destroy_slot(slot);
  }
  if (!capture_pass(e, enqueue, &slot.graph, &slot.exec)) {
    e->graph_failed = true;
    if (hipStreamSynchronize(e->stream) != hipSuccess) (void)hipGetLastError();
    drop_graph(e);
    e->graph_table.count_launch();
    return enqueue();   // nothing was executed by the capture
  }
  return e->check(hipGraphLaunch(slot.exec, e->stream), "hipGraphLaunch");
}

}  // namespace

// The forward pass of a run (with P3HIP_FLAG_SYMMETRY_AVG: expand, forward and reduce): one captured graph for the full
// static batch when the engine was created with P3HIP_FLAG_LAUNCH_GRAPH (the reference's TensorRT engine replays a
// captured graph, trt_engine.cc:260-303), the kernel-by-kernel launches otherwise and for every other position count.
// The first full-batch run goes out kernel by kernel (the launchers set their kernels' LDS attributes on first use,
// which a capture must not see), the second is captured, the rest replay.  A capture that fails falls back to the
// launches for good.  Calibration runs (the fp16 plan + absmax) go kernel by kernel.
// P3HIP_FLAG_LAUNCH_GRAPH_ANY: a graph per key instead, run_pass_any above.
bool run_pass(p3hip_engine* e, const Pass& p) {
  e->last_npos = e->sym_slot ? std::max(sym_rows_of(e, p.npos), 0) : p.npos * (e->sym ? e->sym_k : 1);
  auto enqueue = [&] { return e->any_sym() ? enqueue_sym(e, p) : enqueue_forward(e, p); };
  if (e->graph_any()) return run_pass_any(e, p, enqueue);
  auto launch = [&] { ++e->graph_launched; return enqueue(); };
  if (!(e->flags & P3HIP_FLAG_LAUNCH_GRAPH) || p.npos != e->batch || e->graph_failed || e->calibrating) return launch();
  // P3HIP_FLAG_SYMMETRY_SLOT: the graph's grids are those of batch forward rows, every slot under one symmetry (the
  // kernels read which from the table in device memory, so it may change from replay to replay); a run with an
  // averaged slot has more rows and goes out kernel by kernel
  if (e->sym_slot && e->last_npos != e->batch) return launch();
  // The capture bakes every kernel argument in: the feature buffer the pass reads (run_cached's passes read the cache's
  // gathered copy) and whether it writes d_res.  The graph serves the pass it was captured for; any other goes out
  // kernel by kernel.
  if (e->graph_exec) {
    if (p.feats != e->graph_pass.feats || p.res != e->graph_pass.res) return launch();
    ++e->graph_replays;
    return e->check(hipGraphLaunch(e->graph_exec, e->stream), "hipGraphLaunch");
  }
  if (!e->graph_warm) {
    e->graph_warm = true;
    return launch();
  }
  if (!capture_pass(e, enqueue, &e->graph, &e->graph_exec)) {
    e->graph_failed = true;
    return launch();   // nothing was executed by the capture
  }
  e->graph_pass = p;
  ++e->graph_captures;
  return e->check(hipGraphLaunch(e->graph_exec, e->stream), "hipGraphLaunch");
}

// Destroys every graph the engine holds; with P3HIP_FLAG_LAUNCH_GRAPH_ANY the table's entries and sightings go too (the
// counters stay).  The caller has drained the stream.
void drop_graph(p3hip_engine* e) {
  if (e->graph_exec) hipGraphExecDestroy(e->graph_exec);
  if (e->graph) hipGraphDestroy(e->graph);
  e->graph_exec = nullptr;
  e->graph = nullptr;
  for (GraphSlot& s : e->graph_slots) destroy_slot(s);
  e->graph_table.clear();
}

}  // namespace eng
