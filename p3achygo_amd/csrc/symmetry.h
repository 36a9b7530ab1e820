// symmetry.h — symmetry-averaged evaluation (P3HIP_FLAG_SYMMETRY_AVG): the D4 index maps of the
// 19 x 19 board and the two kernels around the forward pass.
//
//   k_sym_expand  n feature records -> n x k records, copy j of slot r at row r k + j is the slot under symmetry
//                 syms[j] exactly as host/features.h FillFeatures would have produced it: the five grids moved by the
//                 forward map (out[fwd[s][i]] = in[i]), every on-board last move through the forward map, pass, noop
//                 and every other off-board location, colour, komi and board size copied.
//   k_sym_reduce  the copies' kOutStride rows -> one row per slot: the board-indexed entries (0..360 of the move logits,
//                 move probabilities, opt-policy logits and probabilities, and the ownership map) rotated back the way
//                 host/symmetry.h ApplyInverse does (out[inv[s][i]] = in[i], i.e. out[p] = in[fwd[s][p]]), then every
//                 float acc = v_0; acc += v_1; ...; acc / (float)k in fp32 with a correctly rounded division.
//
// P3HIP_FLAG_SYMMETRY_SLOT: the same rule with a mask per slot.  The copies of dense slot r lie at
// rows first[r] .. first[r] + k_r - 1 (k_r the popcount of the slot's mask, ascending symmetry), first[] the running sum
// of the popcounts (sym_rows), so a run of n slots is `total` = first[n - 1] + k_{n-1} forward rows.
//
//   k_sym_expand_slots  n feature records -> total records, slot r's copies from row first[r] on
//   k_sym_reduce_slots  the total rows -> one row per slot
//
// Both read first[] and the masks from device memory (uploaded with the features), so a captured graph whose grids are
// fixed (every k_r = 1) serves whatever symmetries the slots carry.  The per-copy bodies are written once for both pairs.
//
// The maps are built here by a constexpr function, once for the kernels (constant memory) and once for
// p3hip_symmetry_maps, so a CPU test pins the very tables the kernels read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace p3 {

constexpr int kSymN = 19;
constexpr int kSymLocs = kSymN * kSymN;
constexpr int kNumSyms = 8;

// cc/game/symmetry.cc TransformIndex / TransformInv (host/symmetry.h restates them with the same enum order:
// identity, rot90, rot180, rot270, flip, flipRot90, flipRot180, flipRot270)
constexpr int sym_rot(int idx, int n, int quarter) {
  const int i = idx / n, j = idx % n;
  return quarter == 1 ? j * n + (n - 1 - i) : quarter == 2 ? (n - 1 - i) * n + (n - 1 - j) : (n - 1 - j) * n + i;
}
constexpr int sym_flip(int idx, int n) { return (idx / n) * n + (n - 1 - idx % n); }
constexpr int sym_forward(int s, int idx, int n) {
  return s == 0 ? idx : s < 4 ? sym_rot(idx, n, s) : s == 4 ? sym_flip(idx, n) : sym_rot(sym_flip(idx, n), n, s - 4);
}
constexpr int sym_inverse(int s, int idx, int n) {
  return s == 0 ? idx : s < 4 ? sym_rot(idx, n, 4 - s) : s == 4 ? sym_flip(idx, n) : sym_flip(sym_rot(idx, n, 8 - s), n);
}

struct SymMaps {
  uint16_t fwd[kNumSyms][kSymLocs];
  uint16_t inv[kNumSyms][kSymLocs];
};
constexpr SymMaps make_sym_maps() {
  SymMaps m{};
  for (int s = 0; s < kNumSyms; ++s)
    for (int i = 0; i < kSymLocs; ++i) {
      m.fwd[s][i] = (uint16_t)sym_forward(s, i, kSymN);
      m.inv[s][i] = (uint16_t)sym_inverse(s, i, kSymN);
    }
  return m;
}

// The symmetries of a mask (bit s = symmetry s) in ascending order; returns k.
inline int sym_list(uint32_t mask, int out[kNumSyms]) {
  int k = 0;
  for (int s = 0; s < kNumSyms; ++s)
    if (mask & (1u << s)) out[k++] = s;
  return k;
}

struct SymExpandArgs {
  const unsigned char* in;   // [n] p3hip_features, dense
  unsigned char* out;        // [n * k] p3hip_features
  int n, k;
  int syms[kNumSyms];        // ascending
};
struct SymReduceArgs {
  const float* rows;   // [n * k][kOutStride]: the heads' output of the copies
  float* out;          // [n][kOutStride]: the averaged rows (d_out)
  float* res;          // [n][kResultFloats] dense result records, or null
  int n, k;
  int syms[kNumSyms];
};

struct SymExpandSlotsArgs {
  const unsigned char* in;     // [n] p3hip_features, dense
  unsigned char* out;          // [cap] p3hip_features
  const int* first;            // [n] first row of the slot's copies
  const unsigned char* mask;   // [n] the slot's symmetries, 1 .. 255
  int n, cap;                  // cap: the rows `out` holds; a table entry that would pass it writes nothing
};
struct SymReduceSlotsArgs {
  const float* rows;   // [cap][kOutStride]
  float* out;          // [n][kOutStride]
  float* res;          // [n][kResultFloats] or null
  const int* first;
  const unsigned char* mask;
  int n, cap;
};

// first[r] = the popcounts of masks[0 .. r - 1] summed, *total = the sum over all n.  1 for n < 1, a mask of 0, or a
// total above `rows`; 0 otherwise.  No device.  The engine builds the table it uploads with this function
// (p3hip_debug_symmetry_rows is this function).
int sym_rows(const uint8_t* masks, int n, int rows, int* first, int* total);

hipError_t launch_sym_expand(const SymExpandArgs& a, hipStream_t s);
// total: the table's sum of copies as sym_rows returned it; hipErrorInvalidValue for n < 1 and for total > cap
hipError_t launch_sym_expand_slots(const SymExpandSlotsArgs& a, int total, hipStream_t s);
hipError_t launch_sym_reduce_slots(const SymReduceSlotsArgs& a, int total, hipStream_t s);
hipError_t launch_sym_reduce(const SymReduceArgs& a, hipStream_t s);
// the tables the kernels read (host copy of the same constexpr build)
void sym_maps(uint16_t fwd[kNumSyms][kSymLocs], uint16_t inv[kNumSyms][kSymLocs]);

}  // namespace p3
