// edge_split.h — the launches around the trunk on the two low-latency plans (include/p3hip.h P3HIP_FLAG_LOW_LATENCY and
// P3HIP_FLAG_LOW_LATENCY_TFM; Path::Split and Path::TfmSplit): split forms of the stem, the broadcast dense and the heads,
// which otherwise give a position to one workgroup (k_heads: four positions) and so run on as many CUs as the run has
// positions, or fewer.
//
//   k_init_split<CP>   the stem (layer_kernels.h init_body): an item is (position, output pass of CP channels).  The item
//                      expands the planes itself, starts the weight ring at its pass of the stream and computes the
//                      game-state bias of its own channels; an output's chain is conv_segment<G, CP, 5, 28>, as in k_init
//                      and k_init_any.
//   k_bdense_split     the broadcast dense (layer_kernels.h bdense_body): an item is (position, 128-channel half, pass jp
//                      of 128 dense columns), or (.., 32-channel tile ct) as well.  Every u[c][j] keeps its K loop over
//                      the board points (conv_segment<GeoTt, 128, 1, 1, true>), its bias and its BN + mish epilogue.
//   k_heads_pool, k_heads_points, k_heads_softmax
//                      k_heads (kernels.hip) in three launches, cut where a value needs another workgroup's: the pooling
//                      (one wave per channel quad, as there) into a small buffer; the small dense layers recomputed by
//                      every workgroup that needs them, then ranges of the 361 board points or of the 800 score bins, each
//                      value computed without a neighbour; the softmaxes, one workgroup per (position, softmax) with
//                      k_heads' thread mapping and combine order, so that the max and the sum are the same floats.
//
// All cut along lines that leave each output value's arithmetic as it is, so the results are those of the unsplit
// kernels bit for bit (tests/test_edge_split_gpu.py compares bytes).  Where the chooser answers 1 the launch IS the unsplit
// kernel (launch_init, launch_init_any, launch_bdense_any, launch_heads).  The passages a split kernel has in common with
// its unsplit one are one text, included by both (stem_*.inc, bdense_*.inc, heads_score_bin.inc); edge_split.hip's head
// says which two of the heads are still written twice.
//
// Plans whose heads are k_headsx (the transformer plans at stream 128 or 256 with V <= 64, b14d96h3_transformer among
// them) keep it: its pooling order is not k_heads', and P3HIP_FLAG_LOW_LATENCY_TFM is pinned to the default plan's bytes.
// Those nets get the split stem only; a forced heads split is ignored there.  k_heads_aux and the head convs stay as
// they are.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace p3 {

constexpr int kHeadsPoolFloats = 128;   // what the split heads pool per position: mean and max of the 32 g and the 32 v channels

// ---- the sets ------------------------------------------------------------------------------------------
// stem:  1, or the stem's output passes: c_pad / 128 where c_pad is a multiple of 128, else c_pad / 64 (the pass width the
//        stem's weight stream is packed for, conv_any.h conv_any_init_pass; the templated k_init's too).  One pass at 64
//        and 128 channels: no split there
// dense: 1, 3 (the passes jp) or 12 (jp x the four channel tiles ct)
// heads: 1, 4 or 8 workgroups per position in k_heads_points (a quarter of them on the board points, the others on the
//        score bins); k_heads_pool then takes 4 and k_heads_softmax 3 per position
inline int edge_stem_pass(int c_pad) { return c_pad % 128 == 0 ? 128 : 64; }
inline int edge_stem_passes(int c_pad) { return c_pad / edge_stem_pass(c_pad); }
inline bool edge_width_ok(int c_pad) { return c_pad >= 64 && c_pad <= 512 && c_pad % 64 == 0; }
inline bool edge_split_valid(int c_pad, int stem, int dense, int heads) {
  return (stem == 1 || (stem > 1 && stem == edge_stem_passes(c_pad))) && (dense == 1 || dense == 3 || dense == 12) &&
         (heads == 1 || heads == 4 || heads == 8);
}

// The parts per position of the three pieces for a launch over npos positions of a c_pad-channel stream on n_cu CUs:
// the finest level whose items (positions x parts; the dense: x the ceil(c_pad / 128) halves as well) fit ONE round of
// the grid, one workgroup per CU, and 1, the unsplit launch, where none does.  The reason is conv_split.h's: an item's
// time at these sizes is the wait for its loads, much the same for a fine and a coarse item, so a second round costs what
// the finer split saved.  More positions never give a finer split.
inline void edge_split(int npos, int c_pad, int n_cu, int* stem, int* dense, int* heads) {
  const int ncp = edge_stem_passes(c_pad), nhalf = (c_pad + 127) / 128;
  *stem = (long)npos * ncp <= n_cu ? ncp : 1;
  *dense = (long)npos * nhalf * 12 <= n_cu ? 12 : (long)npos * nhalf * 3 <= n_cu ? 3 : 1;
  *heads = (long)npos * 8 <= n_cu ? 8 : (long)npos * 4 <= n_cu ? 4 : 1;
}

// ---- the launchers ---------------------------------------------------------------------------------------
// C: the stream's width, a multiple of 64 up to 512.  parts > 1 and of the sets above; the items are dealt round over at
// most n_cu workgroups.
hipError_t launch_init_split(int C, const InitArgs& a, int parts, int n_cu, hipStream_t s);
hipError_t launch_bdense_split(int C, const BDenseArgs& a, int parts, int n_cu, hipStream_t s);
// k_heads' launch in three; pooled: [a.npos][kHeadsPoolFloats] floats of scratch; a.V up to 80; parts 4 or 8
hipError_t launch_heads_split(const HeadsArgs& a, float* pooled, int parts, hipStream_t s);

}  // namespace p3
