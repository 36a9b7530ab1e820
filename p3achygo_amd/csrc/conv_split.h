// conv_split.h — the low-latency plan of the conv trunks (include/p3hip.h P3HIP_FLAG_LOW_LATENCY): one layer conv,
// k_sconv<KW>, that splits a position across many workgroups, for runs of a few positions that would otherwise occupy
// as many CUs as they have positions.  Widths are launch arguments, multiples of 64 channels (WeightFile::pad_conv pads a
// file's C and C_b); activations are the engine's [pos][C / 8][361][8] fp16.
//
// A work item is (position, tile of T output channels, strip of board rows): S strips of ceil(19 / S) rows, the last one
// shorter (S = 2: 10 + 9 rows, S = 4: 5 + 5 + 5 + 4).  An item stages its rows of the input (with one halo row on each
// side for a 3x3), runs the whole K loop and stores its own outputs: no K split, no atomics, no second pass.  Every
// output is the same chain of MFMAs whatever (S, T), so the split never changes a bit of the result.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace p3 {

constexpr int kSplitMaxC = 512;

// One conv of the layer-wise plan (the flags of LConvArgs), and the two 1x1 convs of a broadcast block as flag sets:
//   y = conv(in') [+ out], in' = mish(bn_in(in)) when pre
//   act 1: mish(bn_out(y)) stored instead of y; act 2: mish(y) (broadcast conv_first)
//   dual: y to `out` and mish(bn_out(y)) to `out2`
// fp32 accumulation, BN, mish and residual add; one rounding to fp16 at each store.
struct SConvArgs {
  const _Float16* in;   // [npos][cin / 8][361][8]
  _Float16* out;        // [npos][cout / 8][361][8]; read as the residual when res
  _Float16* out2;
  int npos, cin, cout;
  const void* w;        // pack_sconv
  int pre, act, res, dual;
  const float *scale_in, *shift_in;    // [cin]
  const float *scale_out, *shift_out;  // [cout]
  int strips, tile;     // the split (sconv_split)
};

// kw 1 or 3; cin, cout multiples of 64 up to kSplitMaxC; (a.strips, a.tile) of the sets below
hipError_t launch_sconv(int kw, const SConvArgs& a, int n_cu, hipStream_t s);
const char* sconv_kernel_name(int kw);

// ---- the split ---------------------------------------------------------------------------------------
inline bool sconv_split_valid(int strips, int tile) {
  return (strips == 1 || strips == 2 || strips == 4) && (tile == 16 || tile == 32 || tile == 64);
}
inline int sconv_strip_rows(int strips) { return (19 + strips - 1) / strips; }

// The split of a launch over npos positions: levels from coarse to fine, each with twice the items of the one before
// (rows and channels halved in turn, so that neither the halo rows an item re-reads nor the weights it re-reads grow
// alone); the finest level whose npos x S x cout / T items still fit one round of the n_cu workgroups the kernel runs
// at a time (one per CU), and (1, 64) where none does.  An item's time at these sizes is the wait for its loads, much
// the same for a fine and a coarse item, so a second round costs what the finer split saved: measured on b14c384btl3
// with the rule "the coarsest split that fills the CUs", 384 items against 192 took a forward pass from 1.33 to 2.06 ms.  More positions never give a finer split, and from
// npos x cout / 64 > n_cu / 2 on it is (1, 64): large runs pay no halo re-reads.  kw is part of the interface (a 1x1
// has no halo) and does not change the choice today.
inline void sconv_split(int npos, int kw, int cout, int n_cu, int* strips, int* tile) {
  static const int level[5][2] = {{1, 64}, {2, 64}, {2, 32}, {4, 32}, {4, 16}};
  (void)kw;
  int l = 4;
  while (l > 0 && (long)npos * level[l][0] * (cout / level[l][1]) > n_cu) --l;
  *strips = level[l][0];
  *tile = level[l][1];
}

// ---- the weight image ----------------------------------------------------------------------------------
// The A operand of v_mfma_f32_16x16x32_f16 is 16 output channels x 32 input channels: lane l holds row l & 15 and the
// eight k values 8 (l >> 4) .. 8 (l >> 4) + 7, the channel group the activations' [..][8] pieces hold.  One fragment is
// 64 lanes x 8 halves = 1 KB:
//   [cout_pad / 16 tiles ct][cin_pad / 32 steps k][taps][64 lanes][8 e]
//       = W[tap][32 k + 8 (lane >> 4) + e][16 ct + (lane & 15)]
// so that an item's tile of T channels is T / 16 consecutive ct, and what one K slice needs of a ct is contiguous.
// W is HWIO flattened as [taps][cin][cout]; rows and columns beyond it are zero.
inline void pack_sconv(std::vector<_Float16>& dst, const float* W, int taps, int cin, int cout, int cin_pad, int cout_pad) {
  for (int ct = 0; ct < cout_pad / 16; ++ct)
    for (int k = 0; k < cin_pad / 32; ++k)
      for (int tap = 0; tap < taps; ++tap)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 8; ++e) {
            const int ci = 32 * k + 8 * (lane >> 4) + e, co = 16 * ct + (lane & 15);
            dst.push_back((_Float16)(ci < cin && co < cout ? W[((size_t)tap * cin + ci) * cout + co] : 0.0f));
          }
}

}  // namespace p3
