/*
 * p3hip.h — C ABI of the MI355X (gfx950) policy/value-net engine.
 *
 * This is the drop-in boundary for the reference's `nn::Engine` virtuals
 * (cc/nn/engine/engine.h:22-43).  Every entry point mirrors one virtual 1:1 so that a
 * ~50-line C++ adapter `HipEngine : nn::Engine` can forward to it.
 * Plain pointers and sizes only; no C++/torch types cross this line.
 *
 *   Engine::LoadBatch(batch_id, GoFeatures)   -> p3hip_load_slot   (engine.h:35)
 *   Engine::RunInference()                    -> p3hip_run         (engine.h:36)
 *   Engine::GetBatch(batch_id, NNInferResult) -> p3hip_get_slot    (engine.h:37)
 *   Engine::GetOwnership(batch_id, own)       -> p3hip_get_ownership (engine.h:38-39)
 *   CreateEngine(kind, path, batch, version)  -> p3hip_create      (engine_factory.cc:56-73)
 *   Engine::~Engine                           -> p3hip_destroy
 *   Engine::kind()/path()                     -> p3hip_kind / p3hip_path (engine.h:32-33)
 *
 * Threading contract (same as the reference): load_slot/get_slot may be
 * called concurrently from many threads, each on its own slot, without locks; p3hip_run is
 * called by one thread at a time and never overlaps get_slot.  A load_slot on a slot that
 * is not part of the running batch may overlap p3hip_run.
 *
 * Which slots a run evaluates: every slot that has been loaded and whose result has not been
 * fetched yet (p3hip_get_slot / p3hip_get_ownership), compacted into a dense batch.  A slot
 * stays in that set until its result is fetched, not merely until a run has picked it up: the
 * reference's infer thread may start a run while a worker's LoadBatch is landing
 * (cc/nn/nn_interface.cc:351-361) and only count that worker as loaded for the NEXT run, which
 * must then still produce its result.  A slot that has not been evaluated by the last run
 * answers p3hip_get_slot with 2.  Every entry point binds the engine's HIP device on the
 * calling thread, so an engine may be driven from any host thread.
 *
 * Error convention: the reference aborts on failure (trt_engine.cc:27-35).  The C ABI
 * returns status codes and keeps a per-engine message (p3hip_last_error); the C++ adapter
 * CHECK-fails on non-zero, reproducing the reference behaviour.
 */
#ifndef P3HIP_H_
#define P3HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3HIP_BOARD_LEN 19
#define P3HIP_NUM_LOCS 361          /* constants::kNumBoardLocs        constants.h:39 */
#define P3HIP_NUM_MOVES 362         /* constants::kMaxMovesPerPosition constants.h:42 */
#define P3HIP_NUM_LAST_MOVES 5      /* constants::kNumLastMoves        constants.h:66 */
#define P3HIP_NUM_VALUE_LOGITS 2    /* constants::kNumValueLogits      constants.h:57 */
#define P3HIP_NUM_SCORE_LOGITS 800  /* constants::kNumScoreLogits      constants.h:60 */
#define P3HIP_NUM_PLANES 15         /* constants::kNumInputFeaturePlanesV1  constants.h:48 */
#define P3HIP_NUM_SCALARS 8         /* constants::kNumInputFeatureScalarsV1 constants.h:54 */

/* Engine::Kind extended with the HIP engine (engine.h:24-30 has 0..4). */
#define P3HIP_KIND_HIP 5

/* game::Loc (cc/game/loc.h:16-22).  pass = {19,0}, noop = {-1,-1} (loc.h:46-47). */
typedef struct p3hip_loc {
  int32_t i;
  int32_t j;
} p3hip_loc;

/* POD mirror of nn::GoFeatures (cc/nn/engine/go_features.h:12-22); fixed 19x19.
 * Colour values: -1 white, 0 empty, +1 black (constants.h:17-27). */
typedef struct p3hip_features {
  int32_t bsize;
  int8_t color;
  float komi;
  int8_t board[P3HIP_NUM_LOCS];
  p3hip_loc last_moves[P3HIP_NUM_LAST_MOVES];
  int8_t stones_atari[P3HIP_NUM_LOCS];
  int8_t stones_two_liberties[P3HIP_NUM_LOCS];
  int8_t stones_three_liberties[P3HIP_NUM_LOCS];
  int8_t stones_laddered[P3HIP_NUM_LOCS];
} p3hip_features;

/* POD mirror of nn::NNInferResult (cc/nn/engine/engine.h:12-20). */
typedef struct p3hip_result {
  float move_logits[P3HIP_NUM_MOVES];
  float move_probs[P3HIP_NUM_MOVES];
  float value_probs[P3HIP_NUM_VALUE_LOGITS]; /* [0]=P(loss) [1]=P(win), side to move */
  float score_probs[P3HIP_NUM_SCORE_LOGITS];
#ifdef __cplusplus
  alignas(16)
#else
  _Alignas(16)
#endif
      float opt_move_probs[P3HIP_NUM_MOVES];
  float err2_outcome;
} p3hip_result;

typedef struct p3hip_engine p3hip_engine;

/* p3hip_create flags */
#define P3HIP_FLAG_NONE 0u
#define P3HIP_FLAG_RUN_ALL_SLOTS 2u /* always run the full static batch (TRT behaviour,
                                       trt_engine.cc:238-304); default compacts to loaded slots */
#define P3HIP_FLAG_SHARED_DEVICE 4u /* several engines keep this GPU busy at once (the self-play host's game groups, the
                                       two players of a match): launches leave out the start-up stagger that only pays
                                       when a launch has the GPU to itself */
#define P3HIP_FLAG_LAUNCH_GRAPH 8u  /* a run over the full static batch replays ONE captured launch graph, as
                                       TrtEngineImpl::RunInference does (trt_engine.cc:260-303); runs over fewer slots
                                       (compaction, cache hits) are launched kernel by kernel.  Same kernels, same results */
#define P3HIP_FLAG_LAUNCH_GRAPH_ANY 131072u /* a captured launch graph for runs of every size.  Implies
                                       P3HIP_FLAG_LAUNCH_GRAPH; both together are this flag.  The engine keeps a table of
                                       graphs keyed by what a capture bakes into kernel arguments and grids: the slot count of
                                       the pass, its forward rows (the slots, slots x k with P3HIP_FLAG_SYMMETRY_AVG, the
                                       staged table's sum with P3HIP_FLAG_SYMMETRY_SLOT), the feature buffer it reads and
                                       its result target.  The first pass of a key goes out kernel by kernel, the second
                                       is captured and launched, later ones replay; a replay runs the launches of the
                                       kernel-by-kernel pass with the same arguments, so every bit is the same.  What the
                                       kernels read from device memory (features, the slot symmetry table, INT8 scales) may
                                       change between replays.  The table holds P3HIP_GRAPH_CACHE graphs (environment at
                                       p3hip_create: 1..1024, default 64; p3hip_create returns NULL for any other value)
                                       and gives up the one replayed longest ago; p3hip_set_symmetries drops them all.
                                       Calibration passes and the passes of an engine stopped by P3HIP_DEBUG_STOP_BLOCK stay
                                       kernel by kernel.  A capture that fails drops the table and the engine launches
                                       kernel by kernel for good.  Composes with everything P3HIP_FLAG_LAUNCH_GRAPH composes
                                       with: every plan, both low-latency flags, both symmetry flags, P3HIP_FLAG_AUX,
                                       P3HIP_FLAG_RUN_ALL_SLOTS, P3HIP_FLAG_SHARED_DEVICE, the NN cache, p3hip_score and
                                       p3hip_loss.  p3hip_forward_resident and p3hip_run read different result targets and
                                       hold a graph each.  A/B switches, read at p3hip_create: P3HIP_GRAPH_MIN_SEEN (a key is
                                       captured on its n-th sighting, 2..64, default 2) and P3HIP_GRAPH_MAX_ROWS (partial
                                       passes of more forward rows are never captured; default 0, no limit).  Measured
                                       against P3HIP_FLAG_LAUNCH_GRAPH alone (README.md): 0.972-1.009x
                                       of its p3hip_run time on partial runs of the low-latency plans, 1.002x in the worst
                                       case for the table.  See p3hip_graph_state and p3hip_graph_stats below */
#define P3HIP_FLAG_INT8 16u         /* calibrated INT8 inference (TensorRT's INT8 engine with a MinMax calibrator,
                                       python/trt_convert.py, cc/nn/engine/trt_calibrator.h): the convs of the layer-wise
                                       blocks run on int8 inputs and weights.  Layer-wise trunks
                                       only: p3hip_create returns NULL for any other trunk (the C = 256 btl trunks have
                                       P3HIP_FLAG_INT8_FUSED).  See p3hip_int8_* below */
#define P3HIP_FLAG_INT8_FUSED 64u   /* calibrated INT8 inference of the trunks that run fused block kernels: C = 256 /
                                       C_b = 128 trunks of btl blocks with 1, 2 or 3 inner layers (b12c256btl3), broadcast
                                       blocks at any interval.  Every btl block is one launch of an int8 block kernel whose
                                       activations stay in LDS ("Fused INT8 blocks"); p3hip_int8_* as
                                       for P3HIP_FLAG_INT8, (inner layers + 2) quantized tensors per btl block.
                                       p3hip_create returns NULL for any other trunk and for both INT8 flags together */
#define P3HIP_FLAG_INT8_C128 128u   /* the same plan for the C = 128 / C_b = 64 trunks of btl blocks with 1, 2 or 3 inner
                                       layers (b12c128btl3, b10c128btl3, small), broadcast blocks at any interval: every
                                       btl block is one launch of k_block_i8<128,64>, two workgroups per CU (DESIGN.md
                                       section 9, "Fused INT8 blocks at C = 128"); p3hip_int8_* as for
                                       P3HIP_FLAG_INT8_FUSED.  p3hip_create returns NULL for any other trunk (nbt, other
                                       widths, classic, transformers) and for any two of the three INT8 flags together */
#define P3HIP_FLAG_INT8_ANY 2048u   /* calibrated INT8 inference whatever the conv trunk, as P3HIP_FLAG_FP32_ANY is full precision
                                       whatever the trunk.  (384, 192) btl / nbt and classic C = 192 take the plan of
                                       P3HIP_FLAG_INT8, (256, 128) btl with 1, 2 or 3 inner layers that of
                                       P3HIP_FLAG_INT8_FUSED, (128, 64) btl with 1, 2 or 3 inner layers that of
                                       P3HIP_FLAG_INT8_C128, each bit-identical to its own flag alone.  Every other trunk of
                                       P3HIP_CONV_SET (nbt at (128, 64) and (256, 128), classic at any C, every padded or
                                       runtime width) runs layer by layer on k_lconv_i8_any, the INT8 layer conv with its
                                       widths as launch arguments, C and C_b zero-padded to multiples of 64 as the fp16 plan
                                       pads them ("INT8 at any width"): the quantized tensors are the
                                       inputs of every conv of the btl (inner layers + 2), nbt (6) and classic (2) blocks; the
                                       raw streams, the stem, the broadcast blocks and the heads are the fp16 engine's.  With
                                       P3HIP_CONV_ANY=1 in the environment the (384, 192) and classic C = 192 trunks run on
                                       k_lconv_i8_any too, with the results of P3HIP_FLAG_INT8 bit for bit.  It sets no
                                       speed target: it is slower than fp16 on every newly served trunk, 0.48-0.62x where
                                       the fp16 plan is the fused block kernel, 0.86-0.96x elsewhere (README.md).  p3hip_int8_* as for P3HIP_FLAG_INT8; composes with the flags that does.
                                       p3hip_create returns NULL for a transformer trunk, together with any of the three
                                       other INT8 flags, and together with P3HIP_FLAG_FP32 / P3HIP_FLAG_FP32_TFM */
#define P3HIP_FLAG_INT8_CONV3 32768u /* calibrated INT8 for the 3x3 convs of the layer-wise blocks only: each layer runs on the
                                       kernel that wins for it ("INT8 for the 3x3 convs only").  Every
                                       1x1 conv, the stem, the broadcast blocks, the heads and the raw residual streams are
                                       the fp16 engine's; a tensor between two layers is int8 when its consumer is a 3x3
                                       conv and fp16 otherwise.  Served: every conv trunk of P3HIP_CONV_SET whose fp16 plan
                                       runs layer by layer: (384, 192) btl / nbt and every padded or runtime width (with
                                       P3HIP_CONV_ANY=1 the templated shapes run on the runtime-width kernels, same bits).
                                       The quantized tensors are the inputs of the 3x3 convs: the inner layers of a btl
                                       block, 4 per nbt block.  A classic trunk has only 3x3 convs: its plan is
                                       P3HIP_FLAG_INT8's (C = 192) or P3HIP_FLAG_INT8_ANY's, bit for bit.  p3hip_int8_* as
                                       for P3HIP_FLAG_INT8; composes with the flags that does.  p3hip_create returns NULL
                                       for a transformer trunk, for the (256, 128) and (128, 64) btl / nbt trunks (their
                                       fp16 plan is the fused block kernel: P3HIP_FLAG_INT8_FUSED, P3HIP_FLAG_INT8_C128 and
                                       P3HIP_FLAG_INT8_ANY serve them), together with any other INT8 flag, with
                                       P3HIP_FLAG_FP32 / P3HIP_FLAG_FP32_TFM and with either low-latency flag.
                                       Measured on one MI355X, engine only, legs interleaved with fp16 (README.md, DESIGN.md
                                       section 9): 0.84x of fp16's forward time on b14c384btl3 at batch 1024 (12.31 against
                                       14.64 ms), 0.87-0.90x on b10c384nbt, b14c320btl3 and b10c512nbt, 0.99x on b12c192btl3;
                                       0.91-1.00x at batch 256 */
#define P3HIP_FLAG_WINOGRAD 65536u   /* every 3x3 conv of the layer-wise blocks as F(2x2, 3x3) Winograd on fp16 MFMAs (k_wconv,
                                       csrc/conv_wino.hip): 2.25 x fewer multiplications per output, no
                                       calibration, fp16 inputs and outputs everywhere.  The weights are transformed from the
                                       file's fp32 values and rounded once to fp16, the input transform runs in two fp16
                                       stages, accumulation and the output transform are fp32.  Every 1x1 conv, the stem, the
                                       broadcast blocks, the heads, the buffers and the layouts are the fp16 plan's own.  The
                                       plan has its own parity bound (tests/winograd_restatement.py): it is a little less
                                       accurate than the default plan and far more than the INT8 plans.  Served: every conv
                                       trunk of P3HIP_CONV_SET whose fp16 plan runs layer by layer: (384, 192) btl / nbt,
                                       classic at every C, every padded or runtime width (with P3HIP_CONV_ANY=1 the templated
                                       shapes take the runtime-width 1x1 kernels, same bits).  Composes with the flags that
                                       do not touch the trunk.  p3hip_create returns NULL for a transformer trunk, for the
                                       (256, 128) and (128, 64) btl / nbt trunks (their fp16 plan is the fused block
                                       kernel), together with any INT8 flag, with P3HIP_FLAG_FP32 / P3HIP_FLAG_FP32_TFM and
                                       with either low-latency flag.  Measured on one MI355X, legs interleaved with fp16
                                       (README.md): as accurate as fp16 (raw outputs 0.0036 against
                                       0.0033 from the fp32 engine on b14c384btl3) and slower, 1.79x of fp16's forward time
                                       on b14c384btl3 at batch 1024, 1.70-2.31x over five nets and two batches */
#define P3HIP_FLAG_SYMMETRY_AVG 32u /* every slot a run evaluates is evaluated under each symmetry of the engine's set
                                       (default: all eight) and the results averaged on the device, rotated back into the
                                       orientation the slot was loaded in.  Needs 8 x batch_size <= 65536.  See
                                       p3hip_set_symmetries below */

#define P3HIP_FLAG_SYMMETRY_SLOT 16384u /* every slot carries its own symmetry mask (p3hip_set_slot_symmetries below; 0x01
                                       after every load): a run evaluates the copies of all its slots packed densely, one
                                       forward row per set bit, and returns every slot's result rotated back into the
                                       orientation it was loaded in and averaged, by the rule of P3HIP_FLAG_SYMMETRY_AVG.
                                       A search hands its leaves' one random symmetry to the engine in place of rotating
                                       features and results on the host, and evaluates a root under all eight in the same
                                       run: one root at 0xFF and 1023 leaves are 1031 forward rows.  The per-row buffers
                                       hold the symmetry_rows of p3hip_create_rows.  p3hip_create returns NULL together
                                       with P3HIP_FLAG_SYMMETRY_AVG, and together with P3HIP_FLAG_AUX for the reason given
                                       there; every other flag, the NN cache, p3hip_score and p3hip_loss's refusal without
                                       P3HIP_FLAG_AUX compose as with P3HIP_FLAG_SYMMETRY_AVG.  With
                                       P3HIP_FLAG_LAUNCH_GRAPH a run over the full static batch whose slots all have one
                                       symmetry (whichever) replays the graph; a run with an averaged slot goes out kernel by
                                       kernel.  Not built: the aux record, ~~a graph for runs with averaged slots~~ (built:
                                       P3HIP_FLAG_LAUNCH_GRAPH_ANY keys its graphs by the forward rows), and on the
                                       host side root masks in self-play (the eval hosts have them: player keys
                                       nn_device_symmetry and nn_root_symmetry_mask) */

#define P3HIP_FLAG_FP32 256u        /* full-precision inference of the conv trunks: every trunk of P3HIP_CONV_SET runs layer by
                                       layer in fp32 from the stem to the heads (csrc/conv_f32.hip).
                                       Weights are packed as fp32, the three head convs included, activations are stored as
                                       fp32, BN fold, mish and residual adds run in fp32, and every product accumulates on
                                       the f32-input MFMA (v_mfma_f32_32x32x2_f32, bit-equal to an fmaf chain): no fp16 value
                                       exists in the pass.  The activation buffers are twice the fp16 plan's.  The other
                                       flags, the NN cache and compaction work as on any engine.  p3hip_create returns NULL
                                       for a transformer trunk (those have P3HIP_FLAG_FP32_TFM) and together with any of the
                                       three INT8 flags */
#define P3HIP_FLAG_FP32_TFM 512u    /* full-precision inference of the transformer trunks: every trunk of
                                       P3HIP_TRANSFORMER_SET runs in fp32 from the stem to the heads
                                       (csrc/transformer_f32.hip; DESIGN.md section 11, "Transformer trunks").  The stem and
                                       the head convs are those of P3HIP_FLAG_FP32 at the stream's width; the six GEMM
                                       matrices of a block are packed as fp32, the residual stream, q, k, v, o, the softmax
                                       numerators and silu(gate) * up are fp32, and every product accumulates on the
                                       f32-input MFMA (v_mfma_f32_16x16x4_f32): no fp16 value exists in the pass.  The
                                       activation buffers are twice the fp16 plan's.  The other flags, the NN cache and
                                       compaction work as on any engine.  p3hip_create returns NULL for a conv trunk when
                                       P3HIP_FLAG_FP32 is not set as well, and together with any of the three INT8 flags */
#define P3HIP_FLAG_FP32_ANY (256u | 512u) /* P3HIP_FLAG_FP32 | P3HIP_FLAG_FP32_TFM: full precision whatever the trunk.  A
                                       conv trunk takes the plan of P3HIP_FLAG_FP32 (bit-identical to that flag alone), a
                                       transformer trunk the plan of P3HIP_FLAG_FP32_TFM */

#define P3HIP_FLAG_AUX 1024u        /* every forward pass also computes the fifteen outputs of the model (python/model.py:1269-1295)
                                       that p3hip_result and p3hip_get_raw do not carry, on the device, one record per
                                       position: p3hip_get_aux below (csrc/heads_aux.hip).  Everything
                                       else the engine returns keeps its bits.  Composes with every trunk and precision plan
                                       (the record is fp32 in all of them), P3HIP_FLAG_RUN_ALL_SLOTS, P3HIP_FLAG_SHARED_DEVICE
                                       and P3HIP_FLAG_LAUNCH_GRAPH.  p3hip_create returns NULL together with
                                       P3HIP_FLAG_SYMMETRY_AVG, and p3hip_cache_enable fails on such an engine */

#define P3HIP_FLAG_LOW_LATENCY 4096u /* a plan for runs of 1 to about 64 positions (a GTP service or an evaluation match with a
                                       few search threads, cc/gtp/service.cc:708-720): every trunk of P3HIP_CONV_SET runs in
                                       fp16, layer by layer, through k_sconv (csrc/conv_split.hip), which splits a position
                                       into row strips and output-channel tiles across many workgroups, where every other
                                       plan gives a position to one workgroup and leaves the other CUs idle.  The stem, the
                                       broadcast dense and the heads are bit-identical to those of the runtime-width plan
                                       (split forms of them where a launch's positions leave CUs idle: csrc/edge_split.hip,
                                       DESIGN.md section 17; P3HIP_EDGE_SPLIT below).  Results are fp16
                                       with the rounding points of the layer-wise plan (DESIGN.md sections 7 and 15), the
                                       same bits at every batch size, in every slot and for every split.  It costs throughput
                                       at large batches.  Measured forward-pass time over the default plan's at batch
                                       1 / 8 / 32, launch graph on both: b12c256btl3 0.84 / 0.87 /
                                       1.20, b14c384btl3 0.97 / 1.06 / 1.63, b15c192_classic 0.95 / 0.98 / 1.41, b12c128btl3
                                       1.17 / 1.19 / 1.44; the default plan is the faster one from batch 32, 8, 16 and 1 on,
                                       by up to 3.8x at batch 256.  Composes with P3HIP_FLAG_RUN_ALL_SLOTS,
                                       P3HIP_FLAG_SHARED_DEVICE, P3HIP_FLAG_LAUNCH_GRAPH, P3HIP_FLAG_SYMMETRY_AVG, P3HIP_FLAG_AUX, the NN cache,
                                       p3hip_score and p3hip_loss.  P3HIP_BLOCKW is ignored.  P3HIP_SPLIT="S,T" in the
                                       environment at p3hip_create forces S row strips (1, 2, 4) and T-channel tiles (16, 32,
                                       64) for every launch (tests, A/B runs).  p3hip_create returns NULL for a transformer
                                       trunk, together with any INT8 flag, together with P3HIP_FLAG_FP32 or
                                       P3HIP_FLAG_FP32_TFM, and for a P3HIP_SPLIT outside those sets */
#define P3HIP_FLAG_LOW_LATENCY_TFM 8192u /* the same for the transformer trunks: every trunk of P3HIP_TRANSFORMER_SET runs
                                       the fp16 plan with the three launches of a block handed to more workgroups
                                       (csrc/transformer_split.hip): the attention of a (position, head)
                                       in S = 1, 2, 3 or 6 parts of its 23 query tiles, qkv and ffn with T = 16, 32 or 64
                                       tokens per workgroup, chosen per launch from the positions it covers and the CUs.
                                       Every query row and token row is computed as the default plan computes it: the
                                       results are the default fp16 plan's, bit for bit, for every split, and where the split
                                       is (1, 64) (on 256 CUs and d96h3: from 43 positions on) the launches are the default
                                       plan's.  The arena and the buffers are the default plan's; the stem and the heads are
                                       bit-identical to the default plan's (a stem of 256 or 384 channels and the heads kernel
                                       k_heads run split where a launch's positions leave CUs idle, csrc/edge_split.hip,
                                       DESIGN.md section 17; k_headsx stays whole), with one small buffer more.
                                       Measured forward-pass time over the default plan's at batch 1 / 8 / 16 / 32, launch
                                       graph on both: b14d96h3_transformer 0.53 / 0.62 / 0.69 / 0.86
                                       (0.309 ms against 0.587 ms at batch 1), a 14-block d192h6 net 0.50 / 0.56 / 0.79 /
                                       1.00; equal times from 64 and 32 positions on, where the split is (1, 64).
                                       Composes with everything the default transformer plan composes with.
                                       P3HIP_TFM_SPLIT="S,T" in the environment at p3hip_create forces one split for every
                                       launch (tests, A/B runs).  p3hip_create returns NULL for a conv trunk when
                                       P3HIP_FLAG_LOW_LATENCY is not set as well, together with any INT8 flag,
                                       P3HIP_FLAG_FP32 or P3HIP_FLAG_FP32_TFM, and for a P3HIP_TFM_SPLIT outside those sets */
#define P3HIP_FLAG_LOW_LATENCY_ANY (4096u | 8192u) /* P3HIP_FLAG_LOW_LATENCY | P3HIP_FLAG_LOW_LATENCY_TFM: the low-latency
                                       plan whatever the trunk.  A conv trunk takes the plan of P3HIP_FLAG_LOW_LATENCY
                                       (bit-identical to that flag alone), a transformer trunk that of
                                       P3HIP_FLAG_LOW_LATENCY_TFM */

/* Transformer trunks (python/model_transformer.py TransformerBlock, a generic_arch of "transformer" blocks) the engine
 * runs: every block has the same embed_dim d and num_heads h, d equals the stem's channels, d is a multiple of 32 with
 * 64 <= d <= 384, the head width d / h is 32 or 64; any block count the .p3w header allows; H = 32 and V what the heads
 * of the residual stream's width serve ({32, 48, 64}; also 80 where the stream is 384 wide, d > 256).  The residual
 * stream is the smallest of 128, 256, 384 channels that holds d.  p3hip_create refuses every other transformer (and
 * INT8 on any transformer), and p3achygo_amd/keras_import.py every other archive, with this wording: */
#define P3HIP_TRANSFORMER_SET \
  "transformer: d a multiple of 32 with 64 <= d <= 384, head width d / heads 32 or 64, every block alike"

/* Conv trunks the engine runs.  (C, C_b) = (128, 64) and (256, 128) run the fused block kernels, (384, 192) and classic
 * C = 192 the templated layer-wise kernels; every other shape of the set runs layer-wise through kernels that take the
 * widths as launch arguments (csrc/conv_any.hip), in fp16, fp32 (P3HIP_FLAG_FP32, csrc/conv_f32.hip) or calibrated INT8
 * (P3HIP_FLAG_INT8_ANY, csrc/lconv_i8_any.hip).  There a file's C and C_b are zero-padded to the next
 * multiple of 64 when the weights are packed (padded channels are exactly 0 everywhere); p3hip_flops_per_position
 * counts the file's own widths, p3hip_debug_x returns the padded stream.  P3HIP_CONV_ANY=1 in the environment at
 * p3hip_create sends (384, 192) and classic C = 192 through those kernels too, with bit-identical results.
 * p3hip_create refuses every other conv trunk with this wording: */
#define P3HIP_CONV_SET \
  "conv: C a multiple of 32 with 64 <= C <= 512; btl (1-3 inner layers) and nbt blocks with C_b a multiple of 16, " \
  "32 <= C_b <= C; classic blocks of two 3x3 convs (C_b ignored); broadcast blocks at any interval >= 2"

/* Creates an engine from a `.p3w` weight file (see p3achygo_amd/netspec.py) for a static
 * batch of `batch_size` slots on HIP device `device_ordinal`.  `version` is the model
 * feature version (engine_factory.cc:37-53; only 1 is supported: 15 planes + 8 scalars).
 * Returns NULL on failure; p3hip_create_error() then holds the reason. */
p3hip_engine* p3hip_create(const char* weights_path, int batch_size, int version,
                           int device_ordinal, uint32_t flags);
/* p3hip_create with the row capacity of a P3HIP_FLAG_SYMMETRY_SLOT engine: symmetry_rows is the number R of forward rows
 * (copies) one run may evaluate, the size of the per-row device buffers.  0 means 8 x batch_size, which always
 * suffices; otherwise batch_size <= R <= 8 x batch_size.  NULL for a non-zero R without the flag and for R above 65536.
 * p3hip_create(...) is p3hip_create_rows(..., 0). */
p3hip_engine* p3hip_create_rows(const char* weights_path, int batch_size, int version, int device_ordinal,
                                uint32_t flags, int symmetry_rows);
const char* p3hip_create_error(void);
void p3hip_destroy(p3hip_engine* e);

int p3hip_kind(const p3hip_engine* e);          /* always P3HIP_KIND_HIP */
const char* p3hip_path(const p3hip_engine* e);  /* path given to p3hip_create */
int p3hip_batch_size(const p3hip_engine* e);

/* LoadBatch: copy the features of one position into pinned staging slot `slot`. */
int p3hip_load_slot(p3hip_engine* e, int slot, const p3hip_features* f);
/* RunInference: H2D of the loaded-and-unfetched slots, one forward pass, D2H of results,
 * stream sync.  Returns 0 on success (also when no slot is pending: nothing is launched). */
int p3hip_run(p3hip_engine* e);
/* GetBatch: copy the results of slot `slot` of the last p3hip_run and mark the slot fetched.
 * Returns 2 if the last run did not evaluate the slot (`out` is left untouched). */
int p3hip_get_slot(p3hip_engine* e, int slot, p3hip_result* out);
/* GetOwnership: tanh ownership map of slot `slot` (the TRT engine leaves this
 * unsupported, trt_engine.cc:353-356; the HIP engine provides it). */
int p3hip_get_ownership(p3hip_engine* e, int slot, float out[P3HIP_NUM_LOCS]);
const char* p3hip_last_error(const p3hip_engine* e);

/* ---- on-device NN cache (extension; the reference caches on the host, above the engine) ----------
 * The reference's NNInterface keeps an LRU cache of NNInferResults per worker thread, keyed by
 * NNKey{color to move, board hash, last moves, komi}; a hit returns the stored result without touching the
 * engine, a miss evaluates under a random symmetry and stores the un-rotated result
 * (cc/nn/nn_interface.cc:93-132, cc/core/lru_cache.h:17-64).  With 288 GB of HBM the table can live beside the
 * engine instead: one table for all workers and games, looked up and filled by the run itself.
 *   p3hip_cache_enable      once after p3hip_create: 2^log2_entries entries of 13.7 KB (key, symmetry, the
 *                           whole result record) in HBM; each key probes 8 consecutive entries, the least
 *                           recently used of them is replaced.
 *   p3hip_load_slot_keyed   LoadBatch with the position's 128-bit key (any digest of the reference's NNKey;
 *                           0/0 = do not cache) and the symmetry (0..7) the features were rotated by.
 *   p3hip_run               evaluates only the keys the table does not hold, serves the rest from HBM, stores
 *                           what it evaluated.  Two slots with the same new key in one run are both evaluated.
 *   p3hip_get_slot_keyed    GetBatch plus the symmetry of the returned result — the stored one on a hit, which
 *                           the caller undoes exactly as the reference's GetBatch(thread, sym) would have when
 *                           the entry was made — and whether it came from the table.
 * Slots loaded with p3hip_load_slot are evaluated and never cached.  Without p3hip_cache_enable the keyed calls
 * behave as the plain ones (every slot is evaluated; the symmetry reported back is the one loaded, from_cache 0).
 * p3hip_cache_stats: lookups, hits, stored entries, table entries. */
int p3hip_cache_enable(p3hip_engine* e, int log2_entries);
int p3hip_load_slot_keyed(p3hip_engine* e, int slot, const p3hip_features* f, uint64_t key_lo, uint64_t key_hi,
                          int symmetry);
int p3hip_get_slot_keyed(p3hip_engine* e, int slot, p3hip_result* out, int* symmetry, int* from_cache);
int p3hip_cache_stats(const p3hip_engine* e, uint64_t out[4]);

/* ---- calibrated INT8 (P3HIP_FLAG_INT8, P3HIP_FLAG_INT8_FUSED, P3HIP_FLAG_INT8_C128, P3HIP_FLAG_INT8_ANY) ------------------------
 * The quantized tensors are the inputs of every conv of the layer-wise blocks (INT8_FUSED, INT8_C128: of the btl blocks), numbered
 * block by block, conv by conv (the order of the block's .p3w convs).  Each has one symmetric activation scale
 * s_a = max |v| / 127.
 *   p3hip_int8_calibrate   one p3hip_run on the fp16 plan (results fetched with p3hip_get_slot as usual) that also
 *                          folds max |v| of every quantized tensor into the engine's running maxima and sets
 *                          s_a = max / 127 from everything observed so far: the MinMax calibrator, called once per
 *                          calibration batch.  With the NN cache on it evaluates every slot and stores nothing.
 *   p3hip_run              on an INT8 engine runs the int8 plan; it fails before any calibration or p3hip_int8_set_scales.
 *   p3hip_int8_scales      returns the number of quantized tensors (-1 without the flag) and copies up to n scales.
 *   p3hip_int8_set_scales  loads a saved calibration (the calibration cache); n must equal that number.
 * New scales take effect in the next run, graph replay (P3HIP_FLAG_LAUNCH_GRAPH) included. */
int p3hip_int8_calibrate(p3hip_engine* e);
int p3hip_int8_scales(const p3hip_engine* e, float* out, int n);
int p3hip_int8_set_scales(p3hip_engine* e, const float* scales, int n);

/* ---- symmetry-averaged evaluation (P3HIP_FLAG_SYMMETRY_AVG) --------------------------------------------------
 * The copies of a slot are ordered by ascending symmetry index s (the enum order of cc/game/symmetry.h: identity, rot90,
 * rot180, rot270, flip, flipRot90, flipRot180, flipRot270).  Copy j is the slot's features under symmetry s_j, as
 * FillFeatures would have built them: the five grids moved by the forward map (out[fwd[s][i]] = in[i]), on-board last
 * moves through the forward map, every other location (pass {19,0}, noop {-1,-1}) and colour, komi, bsize copied.
 * After the forward pass the board-indexed outputs of every copy are rotated back with the inverse map (entries
 * 0..360 of the move logits, move probabilities, opt-policy logits and opt-policy probabilities, and the ownership
 * map; out[inv[s][i]] = in[i]); then every float of the output row is acc = v_0; acc += v_1; ...; acc / (float)k in
 * fp32, correctly rounded.  p3hip_get_slot, p3hip_get_slot_keyed, p3hip_get_ownership and p3hip_get_raw return that
 * average.  With one symmetry in the set the result is that copy itself.
 *   p3hip_set_symmetries  bit s of mask selects symmetry s; 1..255.  Fails on 0, above 255, and on an engine created
 *                         without the flag.  Applies from the next run.
 *   p3hip_symmetry_maps   the forward and inverse index maps of the 19 x 19 board the kernels use.  Needs no device. */
int p3hip_set_symmetries(p3hip_engine* e, uint32_t mask);
void p3hip_symmetry_maps(uint16_t fwd[8][361], uint16_t inv[8][361]);

/* ---- a symmetry set per slot (P3HIP_FLAG_SYMMETRY_SLOT) -------------------------------------------------------
 * The rule above with a mask per slot.  The copies of the r-th slot of a run (dense, in slot order) occupy the forward
 * rows first[r] .. first[r] + k_r - 1 in ascending symmetry index, first[r] the sum of the popcounts k of the slots in
 * front of it.  Copy j is the slot under symmetry s_j as above; after the forward pass its board-indexed outputs are
 * rotated back, and every float is acc = v_0; acc += v_1; ...; acc / (float)k_r in fp32.  With k_r = 1 the result is
 * that copy rotated back, bit for bit (x / 1.0f is exact): what FillFeatures under s, a plain engine and
 * UnapplySymmetry return.
 *   p3hip_set_slot_symmetries  bit s of mask selects symmetry s.  Sets the mask of the position last loaded into `slot`:
 *                              call it after the load and before the run, from the thread that loaded the slot (the
 *                              threading of p3hip_load_slot).  Every p3hip_load_slot / p3hip_load_slot_keyed resets the
 *                              slot's mask to 0x01, and a slot never loaded has 0x01 (P3HIP_FLAG_RUN_ALL_SLOTS).  The
 *                              features are loaded in the caller's own orientation; p3hip_get_slot,
 *                              p3hip_get_slot_keyed, p3hip_get_ownership and p3hip_get_raw answer in that orientation.
 *                              The NN cache stores that result with the symmetry given to p3hip_load_slot_keyed.
 *                              Returns 1 (message naming the flag) on an engine created without the flag, 1 for a bad
 *                              slot and for a mask of 0 or above 255.  p3hip_set_symmetries fails on such an engine.
 *   p3hip_run                  (p3hip_int8_calibrate, p3hip_upload) returns 1 before anything is launched when the
 *                              masks of its slots add up to more than symmetry_rows copies; the message states the
 *                              sum and the capacity.  No slot has a result then (p3hip_get_slot answers 2) and all of
 *                              them stay pending: lower masks and run again.
 *   p3hip_debug_symmetry_rows  the table the engine uploads for n dense slots with these masks, by the function the
 *                              engine itself calls: first[r], and *total = the sum of the popcounts.  Returns 1 for
 *                              n < 1, any mask of 0, and a total above `rows`.  Needs no device. */
int p3hip_set_slot_symmetries(p3hip_engine* e, int slot, uint32_t mask);
int p3hip_debug_symmetry_rows(const uint8_t* masks, int n, int rows, int* first, int* total);

/* ---- the model's other fifteen outputs (P3HIP_FLAG_AUX) -------------------------------------------------------
 * The network has 25 named outputs (python/model.py:1269-1295, exported by python/scripts/convert_to_onnx.py:462-488 as
 * "00:pi_logits" .. "24:mcts_dist_probs").  Ten reach the caller through p3hip_result and p3hip_get_raw (00-07, 12, 22);
 * an engine created with P3HIP_FLAG_AUX computes the other fifteen in every forward pass (k_heads_aux, fp32 in every
 * precision plan) and keeps one record of P3HIP_AUX_LEN floats per position on the device:
 *   [0..361]    08:pi_logits_aux     channel 1 of policy.out_moves over the activated p; [361] the pass, out_pass[1] - 3
 *   [362..723]  21:pi_logits_soft    policy.soft_moves over p; [723] the pass, soft_pass - 3
 *   [724..726]  09:q6 10:q16 11:q50  tanh(go[2..4]), go = oq_out(mish(oq_embed(pooled v)))
 *   [727..728]  13:q16_err 14:q50_err                    4 sigmoid(go[6..7])   (12:q6_err stays where it is: p3hip_result
 *                                                                              err2_outcome, p3hip_get_raw [1887])
 *   [729..731]  15:q6_score 16:q16_score 17:q50_score    go[8..10]
 *   [732..734]  18:q6_score_err 19:q16_score_err 20:q50_score_err   |go[11..13]|
 *   [735..785]  23:mcts_dist_logits  value.mcts_dist(emb), 51 bins
 *   [786..836]  24:mcts_dist_probs   their softmax
 *   p3hip_get_aux  the record of `slot` from the last run.  1 on an engine without the flag and for a bad slot; 2 when
 *                  the last run did not evaluate the slot (`out` is left untouched), which includes every run of an engine
 *                  stopped in front of the heads (P3HIP_DEBUG_STOP_BLOCK).  Like p3hip_get_raw it maps the slot to its row
 *                  of the run (compaction, P3HIP_FLAG_RUN_ALL_SLOTS) and does not mark the slot fetched.
 * Symmetry averaging is refused: a mean of tanh, |.| and softmax outputs over symmetries is nothing the reference
 * defines.  The NN cache is refused: its table holds output rows that have no room for the record. */
#define P3HIP_AUX_LEN 837
int p3hip_get_aux(p3hip_engine* e, int slot, float out[P3HIP_AUX_LEN]);

/* ---- scoring against labels on the device (nn::Benchmark + DefaultStats, cc/nn/engine/benchmark_engine.cc:25-109) ----
 * The reference judges an engine on labelled positions of a recorded chunk (GoDataset, go_dataset.cc:32-123) by fetching
 * every NNInferResult and updating DefaultStats on the host.  Here the labels go to the device and two small kernels
 * (csrc/score.hip) compute the per-position terms and their sums from the output rows the heads left in HBM: a scoring
 * run needs no p3hip_get_slot per position and no host loop.  The output rows are fp32 in every precision plan.
 *
 * p3hip_labels mirrors nn::GoLabels as far as DefaultStats reads it (go_dataset.h; did_win = score_margin >= 0).
 * The six terms of one position are exactly DefaultStats::Update (benchmark_engine.cc:25-61), quirks included:
 *   argmax        the sequential scan of benchmark_engine.cc:11-22: starts at -FLT_MAX, index 0, advances on strict >.
 *                 So: the lowest index among the largest non-NaN values above -FLT_MAX; index 0 if there is none
 *                 (an all-NaN row, a row of -FLT_MAX or -inf).
 *   [0] policy_loss   -log(p) rounded to float once (taken in double on the device), p = move_probs[argmax(labels.policy)];
 *                     16 when p == 0 (:37-39)
 *   [1] outcome_loss  the same on value_probs[did_win] (:40-43)
 *   [2] policy_hit    1 when argmax(move_probs) == argmax(labels.policy), else 0 (:54-55)
 *   [3] outcome_hit   1 when argmax(value_probs) == did_win, else 0 (:56-58)
 *   [4] score_diff    fabsf(score_margin - (float)score_pred) (:59-60)
 *   [5] score_pred    `int score_pred = Argmax(score_probs) + 0.5 - kScoreInflectionPoint` (:30-31): the double is
 *                     truncated toward zero, so argmax 400 gives 0 and argmax 399 gives 0 as well (-0.5 truncates to 0),
 *                     argmax 0 gives -399, argmax 799 gives 399.  Kept as the reference has it.
 * The reference keeps running means (:45-60); p3hip_score returns sums in double and the count, mean = sum / n.
 *
 *   p3hip_load_labels  the labels of the position last loaded into `slot`.  They belong to that load: a new
 *                      p3hip_load_slot / p3hip_load_slot_keyed of the slot clears them.  Same threading as load_slot.
 *   p3hip_score        scores the rows of the LAST p3hip_run (or p3hip_int8_calibrate) whose slot has labels: gathers
 *                      the labels by output row, uploads them, launches k_score_rows and k_score_sum on the engine's
 *                      stream, waits, and copies back the six sums and the term rows.  Works whether or not the slots
 *                      have been fetched already, until the next run; composes with compaction (row != slot),
 *                      P3HIP_FLAG_RUN_ALL_SLOTS (slots without labels are left out), the NN cache (rows served from
 *                      the table are scored like evaluated ones) and P3HIP_FLAG_SYMMETRY_AVG (the averaged rows are
 *                      scored).  *n_scored = 0 and all sums 0 when no evaluated slot has labels.  The sums are a
 *                      fixed-order reduction: the same rows give the same bits.  Called like p3hip_run: by one thread,
 *                      never overlapping a run.  Fetches nothing: the slots stay pending for p3hip_get_slot.
 *                      A slot that was loaded again after the run is left out (its labels would be the new
 *                      position's, its row the old one's).  The hooks that overwrite the output rows without a run
 *                      (p3hip_forward_resident, p3hip_time_trunk_kernel, p3hip_debug_score_rows) end the last run's
 *                      scoring like a run does: p3hip_score then scores nothing until the next p3hip_run.
 *   p3hip_get_score    the six terms of `slot` from the last p3hip_score; 2 if that call did not score the slot (no
 *                      labels, not evaluated, or a run since).
 *   p3hip_debug_score_rows  test hook: writes n synthetic rows (move_probs [n][362], value_probs [n][2], score_probs
 *                      [n][800]) into output rows 0 .. n - 1 of the engine, scores them against labels[0 .. n - 1] and
 *                      returns terms [n][6] and the six sums.  1 <= n <= batch size.  It overwrites the last run's
 *                      results on the device: run again before fetching ownership or raw outputs. */
typedef struct p3hip_labels {
  float policy[P3HIP_NUM_MOVES];
  float score_margin;
  int32_t did_win;
} p3hip_labels;
#define P3HIP_NUM_SCORE_TERMS 6 /* policy_loss, outcome_loss, policy_hit, outcome_hit, score_diff, score_pred */
int p3hip_load_labels(p3hip_engine* e, int slot, const p3hip_labels* labels);
int p3hip_score(p3hip_engine* e, double sums[P3HIP_NUM_SCORE_TERMS], int* n_scored);
int p3hip_get_score(p3hip_engine* e, int slot, float terms[P3HIP_NUM_SCORE_TERMS]);
int p3hip_debug_score_rows(p3hip_engine* e, const float* move_probs, const float* value_probs, const float* score_probs,
                           const p3hip_labels* labels, int n, float* terms, double sums[P3HIP_NUM_SCORE_TERMS]);

/* ---- the trainer's validation losses on the device (python/model.py:1297-1572, python/train.py:1038-1160) -----------
 * What the reference's trainer logs per generation for a net is P3achyGoModel.compute_losses + v1_loss_terms over
 * validation batches.  An engine created with P3HIP_FLAG_AUX holds every prediction those read on the device (the output
 * rows and the aux records, fp32 in every precision plan); with the targets of a recorded position (p3hip_targets, built
 * by host/tf_reader.h exactly as python/transforms.py _parse_example / _expand_common build GroundTruth) two kernels
 * (csrc/loss.hip) compute the per-position terms and their sums.  Means, the two batch-level clips, the weights of
 * python/loss_coeffs.py and the total are the host's (p3achygo_amd/dataset.py loss_from_sums).
 *
 * What is not mirrored: the trainer's `expand` draws a random symmetry per example and masks the last moves of 5 % of
 * them (transforms.py:222, :424); the engine evaluates a position as recorded, so its number is the identity-symmetry
 * number.  The L2 regulariser (model.losses) needs the raw kernels and is left out.
 *
 * The 19 terms of one position (P3HIP_LOSS_*).  KLD(t, p) is keras.metrics.kl_divergence: both arguments clipped to
 * [1e-7f, 1], then sum t log(t / p); the clip is part of the definition (a peaked softmax has entries below it, a one-hot
 * target contributes 361 terms of 1e-7 log(1e-7 / p)).  Huber is Keras' default, delta = 1.  The arithmetic is double
 * on the device, every term rounded to float once.
 *   [0]  policy             KLD(policy, softmax(pi_logits))                                        model.py:1304-1308
 *   [1]  policy_aux_dist    has_pi_aux_dist * KLD(policy_aux_dist, softmax(pi_logits_aux))          :1314-1322
 *   [2]  policy_aux_scalar  (1 - has_pi_aux_dist) * clip(-log_softmax(pi_logits_aux)[policy_aux], 0, 50)  :1325-1327
 *   [3]  outcome            -sum g log_softmax(outcome_logits); g = [0,1] for score_margin > 0, [1,0] for < 0, else
 *                           [.5,.5] (transforms.py:413-421)
 *   [4..6] q6, q16, q50     (target - prediction)^2                                                :1331-1333
 *   [7]  score_pdf          -log_softmax(score_logits)[k], k = clamp((int)floor(score_margin) + 400, 0, 799)
 *                           (transforms.py:244-256)
 *   [8]  score_cdf          sum_j (H[j >= k] - cumsum(softmax(score_logits))_j)^2                   :1340-1348
 *   [9]  own                mean over 361 points of (own - ownership)^2                            :1351-1352
 *   [10] gamma_sq           gamma^2 (w_gamma is the host's)                                        :1354-1357
 *   [11] q_err              mean of three Huber((q_pred - q)^2, q_err_pred)                        :1465-1472
 *   [12] q_score            mean of three Huber(q_score / 10, q_score_pred / 10)                   :1478-1486
 *   [13] q_score_err        mean of three Huber((q_score_pred - q_score)^2 / 100, q_score_err_pred / 100)  :1493-1511
 *   [14] pi_soft            KLD(policy^0.25 / sum policy^0.25, softmax(pi_logits_soft))            :1518-1527
 *   [15] pi_optimistic      KLD(policy, softmax(pi_logits_optimistic)) * clip(sigmoid(3 (z - 1)), 0, 1), z the weighted
 *                           mean of (q - q_pred) / sqrt(q_err_pred + 1e-6f) with c = 4/7 {3, 1.5, .75}, over 3  :1531-1564
 *   [16] mcts_dist          has_mcts_value_dist * KLD(counts / max(sum counts, 1), softmax(mcts_dist_logits))  :1382-1393
 *   [17] move_hit           argmax(pi_logits) == argmax(policy), the first maximum as argmax has it  train.py:1140-1144
 *   [18] outcome_hit        (argmax(outcome_logits) == 1) == (score_margin >= 0)                   train.py:1146-1150
 *
 *   p3hip_load_targets  the targets of the position last loaded into `slot`; they belong to that load, as labels do
 *                       (p3hip_load_slot / p3hip_load_slot_keyed clear them).  Accepted on any engine.  1 for a bad slot
 *                       and for policy_aux outside 0 .. 361.  Same threading as p3hip_load_slot.
 *   p3hip_loss          the terms of the rows of the LAST p3hip_run (or p3hip_int8_calibrate) whose slot has targets, and
 *                       their 19 sums in double; everything p3hip_score says about rows, compaction,
 *                       P3HIP_FLAG_RUN_ALL_SLOTS, reloaded slots, the hooks that end a run's scoring, the fixed-order sums
 *                       and threading holds here word for word.  Fetches nothing.  Needs P3HIP_FLAG_AUX: 1 on any other
 *                       engine, with a message that names the flag.
 *   p3hip_get_loss      the 19 terms of `slot` from the last p3hip_loss; 2 if that call did not handle the slot.
 *   p3hip_debug_loss_rows  test hook: writes n synthetic raw-output rows (p3hip_get_raw's layout, [n][P3HIP_RAW_LEN]) to
 *                       their places in output rows 0 .. n - 1 and n aux records ([n][P3HIP_AUX_LEN]), runs the same
 *                       kernels against targets[0 .. n - 1] and returns terms [n][19] and the sums.  1 <= n <= batch
 *                       size.  Ends the last run's scoring, as p3hip_debug_score_rows does. */
typedef struct p3hip_targets {
  float policy[P3HIP_NUM_MOVES];
  float policy_aux_dist[P3HIP_NUM_MOVES];
  float own[P3HIP_NUM_LOCS];            /* from the side to move: negated for white (transforms.py:452) */
  float mcts_value_dist[51];            /* visit counts per value bucket, as floats */
  float score_margin, q6, q16, q50, q6_score, q16_score, q50_score;
  int32_t policy_aux;                   /* 0 .. 361, 361 the pass */
  int32_t has_pi_aux_dist, has_mcts_value_dist;
} p3hip_targets;                        /* 1146 x 4 bytes */
#define P3HIP_NUM_LOSS_TERMS 19
int p3hip_load_targets(p3hip_engine* e, int slot, const p3hip_targets* targets);
int p3hip_loss(p3hip_engine* e, double sums[P3HIP_NUM_LOSS_TERMS], int* n);
int p3hip_get_loss(p3hip_engine* e, int slot, float terms[P3HIP_NUM_LOSS_TERMS]);
int p3hip_debug_loss_rows(p3hip_engine* e, const float* raw, const float* aux, const p3hip_targets* targets, int n,
                          float* terms, double sums[P3HIP_NUM_LOSS_TERMS]);

/* ---- measurement / test hooks (not part of the reference surface) ------------------ */

/* Device-resident benchmark step: runs the forward pass on whatever is already staged in
 * HBM for `n_positions` slots, no H2D/D2H, no sync.  Used by bench.py's timed region. */
int p3hip_forward_resident(p3hip_engine* e, int n_positions);
/* Upload all currently loaded slots to HBM without running (pairs with the above). */
int p3hip_upload(p3hip_engine* e);
int p3hip_sync(p3hip_engine* e);
/* Raw head outputs of the last run for one slot, for parity tests:
 * out[0..361] pi_logits, [362..723] opt logits, [724..725] outcome logits,
 * [726..1525] score logits, [1526..1886] ownership, [1887] q6_err, [1888] gamma. */
#define P3HIP_RAW_LEN 1889
int p3hip_get_raw(p3hip_engine* e, int slot, float* out);
/* Times the dominant trunk kernel in place: runs `iters` forward passes over the resident
 * batch with a HIP event pair on the engine's stream around every fused-block launch and
 * returns the average milliseconds per launch (<0 on error; also <0 for layer-wise trunks,
 * which have no fused block kernel); writes the
 * algorithmic FLOPs of the convs one launch executes (inner 3x3s + 1x1 reduce/expand,
 * unpadded 361 points).  Transformer trunks: times the attention kernel k_tfm_attn and writes the FLOPs of its
 * q.k^T and p.v products over 361 x 361 tokens.  Layer-wise trunks: times the 3x3 layer conv, k_lconv<3,..>, or on an
 * INT8 engine k_lconv_i8<3,..> (P3HIP_FLAG_INT8_ANY on a trunk of its own path: k_lconv_i8_any<3>, and the FLOPs at the file's own
 * widths), and writes the FLOPs of one 3x3 conv.  A P3HIP_FLAG_FP32 engine is layer-wise whatever its
 * trunk: it times k_lconv_f32<3> and writes the FLOPs of one 3x3 conv at the file's own widths; so is a
 * P3HIP_FLAG_LOW_LATENCY engine, with k_sconv<3>; a P3HIP_FLAG_WINOGRAD engine times k_wconv and writes the FLOPs of one
 * direct 3x3 conv at the file's own widths.  A P3HIP_FLAG_LOW_LATENCY_TFM engine times the attention launch of the
 * split in force for n_positions: k_tfm_attn_split, or k_tfm_attn where that is one part, with the same FLOPs. */
double p3hip_time_trunk_kernel(p3hip_engine* e, int n_positions, int iters,
                               double* flops_per_launch, const char** kernel_name);
/* Test hook, no device: loads the file and builds the host-side plan of (file, flags, the P3HIP_* environment) as
 * p3hip_create would.  Returns the name of the trunk path chosen ("Fused", "Layerwise", "ConvAny", "Int8", "Int8Fused256",
 * "Int8Fused128", "Int8Any", "F32Conv", "Winograd3", "Tfm", ..), or NULL with the reason in p3hip_create_error().  n_q: the quantized
 * tensors of an INT8 plan (0 otherwise); digest: a 64-bit FNV-1a hash over the int8 weight bytes and the weight scales
 * of every quantized conv, in the plan's order (0 without any).  Either pointer may be NULL. */
const char* p3hip_debug_plan(const char* weights_path, uint32_t flags, int* n_q, uint64_t* digest);
/* Test hooks, no device (P3HIP_FLAG_LOW_LATENCY).  p3hip_debug_split: the row strips and the output-channel tile a
 * k_sconv launch of kernel size kw over npos positions and cout output channels takes on a device of n_cu CUs, the
 * P3HIP_SPLIT override included; 0, or 1 for a bad argument or a bad P3HIP_SPLIT.  p3hip_debug_pack_sconv: the kernel's
 * weight image (csrc/conv_split.h pack_sconv) of W[taps][cin][cout] padded to cin_pad x cout_pad (multiples of 64), as
 * raw fp16 bits; returns the number of elements, writes at most n of them. */
int p3hip_debug_split(int npos, int kw, int cout, int n_cu, int* strips, int* tile);
long p3hip_debug_pack_sconv(const float* w, int taps, int cin, int cout, int cin_pad, int cout_pad, uint16_t* out, long n);
/* Test hooks, no device (P3HIP_FLAG_WINOGRAD).  p3hip_debug_pack_wconv: k_wconv's weight image (csrc/conv_wino.h
 * pack_wconv) of the 3x3 conv W[9][cin][cout] padded to cin_pad x cout_pad (multiples of 64), as raw fp16 bits; returns
 * the number of elements, writes at most n of them.  p3hip_debug_wconv_grid: how the launcher cuts a k_wconv launch over
 * npos positions and cout output channels on a device of n_cu CUs (csrc/conv_wino.h wconv_grid, wconv_unit, the
 * functions the launcher and the kernel call): *grid workgroups, *units units of work, dealt round (workgroup b takes
 * the units b, b + grid, ..); with 0 <= unit < units also that unit's first flat tile (tile f = 100 position + 10 tile
 * row + tile column), its tile count and its first output channel (any of the three pointers may be NULL).  Returns 0,
 * or 1 for a bad argument. */
long p3hip_debug_pack_wconv(const float* w, int cin, int cout, int cin_pad, int cout_pad, uint16_t* out, long n);
int p3hip_debug_wconv_grid(int npos, int cout, int n_cu, int* grid, long* units, long unit, long* tile0, int* ntiles, int* cout0);
/* Test hook, no device (P3HIP_FLAG_LOW_LATENCY_TFM): the query parts per (position, head) of the attention launch and the
 * tokens per workgroup of the qkv and ffn launches over npos positions of a trunk with `heads` heads on a device of n_cu
 * CUs, the P3HIP_TFM_SPLIT override included; 0, or 1 for a bad argument or a bad P3HIP_TFM_SPLIT. */
int p3hip_debug_tfm_split(int npos, int heads, int n_cu, int* parts, int* tokens);
/* Test hook, no device (both low-latency flags): the parts per position of the stem, the broadcast dense and the heads
 * launches over npos positions of a stream of c_pad channels (a multiple of 64 up to 512) on a device of n_cu CUs
 * (csrc/edge_split.h), the P3HIP_EDGE_SPLIT override included.  stem: 1 or the stem's output passes
 * (c_pad / 128, or c_pad / 64 where c_pad is no multiple of 128); dense: 1, 3 or 12; heads: 1, 4 or 8 (ignored where
 * the heads kernel is k_headsx).  A part count of 1 is the unsplit launch.  Returns 0, or 1 (and 1, 1, 1) for a bad argument or a P3HIP_EDGE_SPLIT outside those sets.
 * P3HIP_EDGE_SPLIT="s,d,h" in the environment at p3hip_create forces the parts of every such launch of an engine with
 * either low-latency flag (tests, A/B runs); "0" forces 1,1,1, the launches of the engine before the split forms existed;
 * p3hip_create returns NULL for any other value.  Without a low-latency flag nothing reads it. */
int p3hip_debug_edge_split(int npos, int c_pad, int n_cu, int* stem, int* dense, int* heads);
/* P3HIP_FLAG_LAUNCH_GRAPH: 1 once the full-batch forward pass has been captured and is being replayed,
 * 0 before (or without the flag), -1 when the capture failed and the engine fell back to plain launches. */
int p3hip_graph_state(const p3hip_engine* e);
/* P3HIP_FLAG_LAUNCH_GRAPH_ANY: p3hip_graph_state answers 0 while no graph is held, 1 once any is, -1 after a failed capture.
 * p3hip_graph_stats fills out[0..4] with the graphs held now and, since p3hip_create, the captures, the replays, the forward
 * passes launched kernel by kernel and the graphs given up for a newer one (evictions; graphs dropped all at once by
 * p3hip_set_symmetries are not counted).  An engine with P3HIP_FLAG_LAUNCH_GRAPH alone reports its single graph (no
 * evictions).  Returns 0, or 1 (and zeroes) on an engine without either flag. */
int p3hip_graph_stats(const p3hip_engine* e, uint64_t out[5]);
/* Test hook, no device: feeds n keys (npos[i], total[i]; feature buffer and result target fixed) through the policy of a
 * P3HIP_FLAG_LAUNCH_GRAPH_ANY engine's table (csrc/graph_table.h) at the given capacity (1..1024).  action[i]: 0 launched
 * kernel by kernel, 1 captured and launched, 2 replayed; evicted[i]: the step whose graph step i's capture gave up, or
 * -1.  Returns 0, or 1 for a bad argument. */
int p3hip_debug_graph_table(const int* npos, const int* total, int n, int capacity, int* action, int* evicted);
/* Diagnostics of the hand-scheduled block kernel k_blockw (engines created with P3HIP_BLOCKW_DIAG in the environment
 * run its _diag twin, which stamps s_memtime at its section boundaries): copies up to n 64-bit stamps of the last
 * forward pass, [workgroup 0..7][block 0..15][wave 0..3][24], to out.  Returns 0, or 1 when there are none. */
int p3hip_blockw_stamps(p3hip_engine* e, unsigned long long* out, int n);
/* Debugging aid: the residual stream x after the last forward pass (stopped early by P3HIP_DEBUG_STOP_BLOCK in the
 * environment, if set), n_positions x C x 361 values in the device layout [pos][C / 8][361][8], as floats.
 * A P3HIP_FLAG_FP32 or P3HIP_FLAG_FP32_TFM engine returns its stored fp32 values, exactly, in the same order.
 * Transformer trunks: C is the stream's padded width (the model's d channels, then the channels up to 128, 256 or 384
 * that stay zero). */
int p3hip_debug_x(p3hip_engine* e, float* out, int n_positions);
/* Test hook, layer-wise INT8 engines (the paths of P3HIP_FLAG_INT8 and of P3HIP_FLAG_INT8_ANY's own plan): the int8
 * activated copy of x that a layer-wise block stores for the layer-wise block behind it, q(mish(bn0(x))) taken from
 * the unrounded fp32 sum, [pos][C / 16][361][16] with the padded C.  Meaningful after a pass stopped in front of such a
 * block (P3HIP_DEBUG_STOP_BLOCK).  Returns 0, 1 on any other engine. */
int p3hip_debug_act_i8(p3hip_engine* e, int8_t* out, int n_positions);
/* Test hook of transformer trunks: what the last transformer block that ran left in device memory, as floats.
 * which 0, 1, 2 = q, k, v as [pos][head][384][D], the 23 padding rows 361..383 of every head included; 3 = the
 * attention output o as [pos][361][d].  It only reads buffers the forward pass owns.  The heads take o's buffer as
 * scratch: o is the last block's only on an engine stopped in front of them (P3HIP_DEBUG_STOP_BLOCK = n ends the pass
 * in front of block n; n = the block count ends it after the last block, in front of the heads).  Returns non-zero for
 * an engine without a transformer trunk, for n_positions < 1 or beyond the last run's, and for any other `which`.
 * A P3HIP_FLAG_FP32_TFM engine returns its stored fp32 values, exactly, in the same orders. */
int p3hip_debug_tfm(p3hip_engine* e, int which, float* out, int n_positions);
/* Test hook: fills with `byte` (0 .. 255), on the engine's stream, every value buffer on the device that a forward pass
 * has to write before it reads it, then waits for the fill: the residual stream and the blocks' scratch, token rows
 * 0 .. 360 of the transformer's q, k and v, the heads' scratch, the output rows, the dense result records and the aux
 * records, and the term and sum buffers of p3hip_score and p3hip_loss where they exist.  An engine that reads no byte it
 * did not write computes the same bits after it as without it (0xFF: NaN as fp16 and fp32, -1 as int8; 0x7B: about
 * 6.1e4 as fp16, 1.3e36 as fp32, 123 as int8).  Left alone: what is state (weights, INT8 maxima and scales, the NN
 * cache's table, labels and targets), every record an address is computed from (features, symmetry tables, the cache's
 * keys and lists, the rows of scoring and loss), and what p3hip_create zeroes once for good (q, k, v rows 361 .. 383).
 * The results of earlier runs are gone: p3hip_get_slot, p3hip_get_ownership, p3hip_get_raw, p3hip_get_aux,
 * p3hip_get_score and p3hip_get_loss answer 2 and p3hip_score / p3hip_loss find no row until the next run; a slot whose
 * result had not been fetched is evaluated again by that run.  A captured launch graph stays valid.  Returns 0, 1 on a
 * bad byte or a HIP error. */
int p3hip_debug_poison(p3hip_engine* e, int byte);
/* Test hook, no device needed: the table p3hip_debug_poison goes by, one line per device buffer of an engine,
 * "member<TAB>class<TAB>range": class is poisoned, state, index or zeroed-once, range the part of a zeroed-once buffer
 * that stays zero ("What a forward pass may read"). */
const char* p3hip_debug_poison_table(void);
/* Algorithmic FLOPs (2*MAC) of one position: total, and 3x3 trunk convs only. */
void p3hip_flops_per_position(const p3hip_engine* e, double* total, double* conv3x3);
/* The spiral RoPE tables the transformer trunk uses (python/model_transformer.py, head_dim 32, 4 rotations, theta
 * 100), [361 tokens][32] each, in double precision.  Needs no device. */
void p3hip_rope_table(double* cos_out, double* sin_out);
/* The same for head width head_dim (32 or 64): [361 tokens][head_dim] each.  Returns 0, or non-zero (tables untouched)
 * for any other width.  Needs no device. */
int p3hip_rope_table_dim(int head_dim, double* cos_out, double* sin_out);

#ifdef __cplusplus
}
#endif
#endif /* P3HIP_H_ */
