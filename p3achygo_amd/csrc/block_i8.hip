// block_i8.hip — the fused INT8 block kernel of the C = 256 / C_b = 128 btl trunks (P3HIP_FLAG_INT8_FUSED).
// Numerics: DESIGN.md section 9 "Fused INT8 blocks"; operand layouts and the lane map of v_mfma_i32_16x16x64_i8 are those
// of lconv_i8.hip (weights in pack_lconv_i8 order, lconv_i8.h).
//
// A workgroup of eight waves owns one position through a whole btl block; the activations never leave the chip
// between the block's convs.  LDS holds two zero-bordered 21 x 21 int8 images of 128 channels each
// ([16-channel group][441 points][16], 56,448 B; 112,896 B together, so one workgroup per CU):
//   stage    x (fp16, 256 channels) -> q(mish(bn0(x))) into both images (channels 0..127 | 128..255), once
//   reduce   1x1, K = 256 over both images; after a barrier its quantizing epilogue writes image 0
//   inner j  3x3, K = 128 from image cur; the quantizing epilogue writes image 1 - cur
//   expand   1x1, K = 128 from image cur, two passes of 64 output channels per wave; + x, stored as fp16
// The input of a layer is staged once, not once per 64-channel output pass.  Wave w takes output channels
// 64 (w & 1) .. + 63 (four 16-channel tiles) and the 16-point tiles (w >> 1) + 4 i of the 23 that cover the board: 96
// accumulator registers.  Per tap and 64-channel K slice it reads four weight fragments from global memory (shared by
// the workgroup's waves through L1, the next step's prefetched under the MFMAs) and six activation fragments from LDS,
// and issues 24 MFMAs.
#include "block_i8.h"
#include "block_i8_core.h"
#include "launch_util.h"

namespace p3 {

namespace {

using namespace i8blk;   // the padded image, the quantizer, stage_pre and a wave's conv_i8 (block_i8_core.h)

constexpr int kImageBytes = 8 * kGroupBytes;    // 128 channels: 56,448
constexpr int kLdsBytes = 2 * kImageBytes;      // 112,896
static_assert(kLdsBytes <= 160 * 1024, "two 128-channel images within the CU's 160 KiB of LDS");
constexpr int kWgB = 512;
constexpr int kC = 256, kCb = 128;
constexpr int kStageItems = (kC / 16) * kNLoc;  // 5,776 sixteen-byte points of a position

template <int L>
__global__ void __launch_bounds__(kWgB) k_block_i8(BlockI8Args a) {
  static_assert(L >= 1 && L + 2 <= kBlockI8MaxConvs, "one to three inner layers");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4;
  const int half = wid & 1, pg = wid >> 1;

  // the border of both images stays zero (only interior points are ever written)
  for (int i = tid; i < kLdsBytes / 16; i += kWgB) *(i32x4*)(smem + 16 * i) = i32x4{0, 0, 0, 0};

  // this lane's board points: tile t = pg + 4 i, point 16 t + (lane & 15); points past the board read the image at
  // point 0's place (any in-range address) and are never stored
  int pidx[kTilesPerWave];
#pragma unroll
  for (int i = 0; i < kTilesPerWave; ++i) {
    const int loc = 16 * (pg + 4 * i) + (lane & 15);
    pidx[i] = (g * kPadPts + (loc < kNLoc ? pad_index(loc) : pad_index(0))) * 16;
  }
  const int ntile = pg + 4 * (kTilesPerWave - 1) < kTiles ? kTilesPerWave : kTilesPerWave - 1;   // wave-uniform

  i32x4 acc[kTilesPerWave][4];
  auto acc_zero = [&]() {
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[i][ct] = i32x4{0, 0, 0, 0};
  };
  // conv j's epilogue for a layer that feeds another conv: q(mish(bn_{j+1}(acc * (s_in * s_w[c])))) into image `out`
  auto store_q = [&](int j, float s_in, float s_out, char* out) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int c0 = half * 64 + ct * 16 + 4 * g;
      const f32x4 sw = *(const f32x4*)(a.w_scale[j] + c0);
      const f32x4 sc = *(const f32x4*)(a.scale[j + 1] + c0), sh = *(const f32x4*)(a.shift[j + 1] + c0);
#pragma unroll
      for (int i = 0; i < kTilesPerWave; ++i) {
        const int loc = 16 * (pg + 4 * i) + (lane & 15);
        if (i >= ntile || loc >= kNLoc) continue;
        unsigned u = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = (float)acc[i][ct][r] * (s_in * sw[r]);
          u |= q8(mish_f(v * sc[r] + sh[r]), s_out) << (8 * r);
        }
        *(unsigned*)(out + (c0 >> 4) * kGroupBytes + pad_index(loc) * 16 + (c0 & 15)) = u;
      }
    }
  };

  __syncthreads();   // zeroed images before the first staged store
#pragma unroll 1
  for (int pos = blockIdx.x; pos < a.npos; pos += gridDim.x) {
    _Float16* x = a.x + (size_t)pos * kC * kNLoc;
    // ---- stage q(mish(bn0(x))): 256 channels into both images ------------------------------------------------
    {
      const float s0 = a.act_scale[a.q0];
#pragma unroll 2
      for (int it = tid; it < kStageItems; it += kWgB) {
        const int gc = it / kNLoc, p = it - gc * kNLoc;
        const h8 lo = *(const h8*)(x + ((size_t)(2 * gc) * kNLoc + p) * 8);
        const h8 hi = *(const h8*)(x + ((size_t)(2 * gc + 1) * kNLoc + p) * 8);
        *(i32x4*)(smem + gc * kGroupBytes + pad_index(p) * 16) = stage_pre(lo, hi, a.scale[0], a.shift[0], gc * 16, s0);
      }
    }
    __syncthreads();
    // ---- reduce 1x1, 256 -> 128 ---------------------------------------------------------------------------------
    acc_zero();
    conv_i8<1, kC / 64>(acc, smem, a.w[0] + (size_t)half * (kC / 64) * 4096 + lane * 16, pidx, ntile);
    __syncthreads();   // every wave has read both images: image 0 is free
    store_q(0, a.act_scale[a.q0], a.act_scale[a.q0 + 1], smem);
    __syncthreads();
    // ---- inner 3x3 layers, ping-pong between the images --------------------------------------------------------
    int cur = 0;
#pragma unroll
    for (int j = 1; j <= L; ++j) {
      acc_zero();
      conv_i8<3, kCb / 64>(acc, smem + cur * kImageBytes, a.w[j] + (size_t)half * (kCb / 64) * 9 * 4096 + lane * 16, pidx, ntile);
      store_q(j, a.act_scale[a.q0 + j], a.act_scale[a.q0 + j + 1], smem + (1 - cur) * kImageBytes);
      __syncthreads();
      cur = 1 - cur;
    }
    // ---- expand 1x1, 128 -> 256, + x ----------------------------------------------------------------------------
    const float s_in = a.act_scale[a.q0 + L + 1];
#pragma unroll 1
    for (int k = 0; k < 2; ++k) {
      const int cp = half + 2 * k;
      acc_zero();
      conv_i8<1, kCb / 64>(acc, smem + cur * kImageBytes, a.w[L + 1] + (size_t)cp * (kCb / 64) * 4096 + lane * 16, pidx, ntile);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int c0 = cp * 64 + ct * 16 + 4 * g;
        const f32x4 sw = *(const f32x4*)(a.w_scale[L + 1] + c0);
#pragma unroll
        for (int i = 0; i < kTilesPerWave; ++i) {
          const int loc = 16 * (pg + 4 * i) + (lane & 15);
          if (i >= ntile || loc >= kNLoc) continue;
          _Float16* o = x + ((size_t)(c0 >> 3) * kNLoc + loc) * 8 + (c0 & 7);
          const h4 old = *(const h4*)o;
          h4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = (_Float16)((float)acc[i][ct][r] * (s_in * sw[r]) + (float)old[r]);
          *(h4*)o = v;
        }
      }
    }
    __syncthreads();   // the images are free for the next position
  }
}

template <int L>
hipError_t launch_t(const BlockI8Args& a, int n_cu, hipStream_t s) {
  static AttrOnce once;   // dynamic LDS above 64 KB needs the attribute, once per kernel and device
  if (hipError_t e = ensure_lds(once, k_block_i8<L>, kLdsBytes); e != hipSuccess) return e;
  const int grid = a.npos < n_cu ? a.npos : n_cu;
  hipLaunchKernelGGL((k_block_i8<L>), dim3(grid), dim3(kWgB), kLdsBytes, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_block_i8(const BlockI8Args& a, int n_cu, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  if (a.inner == 1) return launch_t<1>(a, n_cu, s);
  if (a.inner == 2) return launch_t<2>(a, n_cu, s);
  if (a.inner == 3) return launch_t<3>(a, n_cu, s);
  return hipErrorInvalidValue;
}

const char* block_i8_kernel_name() { return "k_block_i8<256,128>"; }

}  // namespace p3
