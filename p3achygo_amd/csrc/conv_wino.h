// conv_wino.h — the Winograd plan of the layer-wise conv trunks (include/p3hip.h P3HIP_FLAG_WINOGRAD): one kernel, k_wconv,
// that runs a 3x3 layer conv as F(2x2, 3x3) Winograd on fp16 MFMAs.  Widths are launch arguments,
// multiples of 64 channels; activations are the engine's [pos][C / 8][361][8] fp16.
//
// A position is 10 x 10 tiles of 2 x 2 outputs; tile (ty, tx) reads the 4 x 4 input patch whose corner is board point
// (2 ty - 1, 2 tx - 1), points outside the board as zeros, and its outputs of row or column 19 are dropped.  The tiles of
// a launch are numbered flat over the positions, tile f = 100 pos + 10 ty + tx, and a unit of work is 32 consecutive tiles
// x 64 output channels: a tile's arithmetic does not depend on the unit it lands in.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace p3 {

constexpr int kWinoTiles = 100;      // tiles of a position
constexpr int kWinoUnitTiles = 32;   // tiles of a unit of work
constexpr int kWinoUnitCout = 64;    // output channels of a unit
constexpr int kWinoMaxC = 512;

// One 3x3 conv of the layer-wise plan, the flags of LConvArgs:
//   y = conv(in') [+ out], in' = mish(bn_in(in)) rounded to fp16 when pre
//   act: mish(bn_out(y)) stored instead of y; dual: y to `out` and mish(bn_out(y)), of the unrounded y, to `out2`
struct WConvArgs {
  const _Float16* in;   // [npos][cin / 8][361][8]
  _Float16* out;        // [npos][cout / 8][361][8]; read as the residual when res
  _Float16* out2;
  int npos, cin, cout;
  const void* w;        // pack_wconv
  int pre, act, res, dual;
  const float *scale_in, *shift_in;    // [cin]
  const float *scale_out, *shift_out;  // [cout]
};

// ---- the cut of a launch -------------------------------------------------------------------------------
// Units of a launch over npos positions and cout channels: unit u is the tile group u / (cout / 64) and the channel
// block u % (cout / 64), so that the units that read the same input tiles are neighbours.  The grid is one workgroup
// per CU at the most (the kernel's registers allow one wave per SIMD); workgroup b takes the units b, b + grid, ..
__host__ __device__ inline long wconv_units(int npos, int cout) {
  return (((long)npos * kWinoTiles + kWinoUnitTiles - 1) / kWinoUnitTiles) * (cout / kWinoUnitCout);
}
inline int wconv_grid(int npos, int cout, int n_cu) {
  const long units = wconv_units(npos, cout);
  return (int)(units < (long)n_cu ? units : (long)n_cu);
}
// unit u of that launch: its first flat tile, its tiles (the last group of a launch is short) and its first channel
__host__ __device__ inline void wconv_unit(int npos, int cout, long u, long* tile0, int* ntiles, int* cout0) {
  const int ncb = cout / kWinoUnitCout;
  const long total = (long)npos * kWinoTiles;
  *tile0 = (u / ncb) * kWinoUnitTiles;
  *ntiles = (int)(total - *tile0 < kWinoUnitTiles ? total - *tile0 : kWinoUnitTiles);
  *cout0 = (int)(u % ncb) * kWinoUnitCout;
}

// ---- the weight image ----------------------------------------------------------------------------------
// U = G g G^T per (cin, cout), G = [[1, 0, 0], [1/2, 1/2, 1/2], [1/2, -1/2, 1/2], [0, 0, 1]], computed in double from the
// file's fp32 weights and rounded once to fp16; plane p = 4 i + j is U[i][j].  The image is the A operand of
// v_mfma_f32_16x16x32_f16 (lane l: output channel l & 15, input channels 8 (l >> 4) .. + 7), one 1 KB fragment per
// (channel tile, K step, plane):
//   [cout_pad / 16 tiles ct][cin_pad / 32 steps k][16 planes p][64 lanes][8 e] = U_p[32 k + 8 (lane >> 4) + e][16 ct + (lane & 15)]
// W is HWIO flattened as [9 taps = 3 ky + kx][cin][cout]; rows and columns beyond it are zero.
inline void pack_wconv(std::vector<_Float16>& dst, const float* W, int cin, int cout, int cin_pad, int cout_pad) {
  static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  for (int ct = 0; ct < cout_pad / 16; ++ct)
    for (int k = 0; k < cin_pad / 32; ++k)
      for (int p = 0; p < 16; ++p)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 8; ++e) {
            const int ci = 32 * k + 8 * (lane >> 4) + e, co = 16 * ct + (lane & 15);
            double u = 0.0;
            if (ci < cin && co < cout)
              for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx)
                  u += G[p >> 2][ky] * (double)W[((size_t)(3 * ky + kx) * cin + ci) * cout + co] * G[p & 3][kx];
            dst.push_back((_Float16)u);
          }
}

// cin, cout multiples of 64 up to kWinoMaxC; act 0 or 1
hipError_t launch_wconv(const WConvArgs& a, int n_cu, hipStream_t s);
const char* wconv_kernel_name();

}  // namespace p3
