// block_i8_c128.hip — the fused INT8 block kernel of the C = 128 / C_b = 64 btl trunks (P3HIP_FLAG_INT8_C128).
// Numerics: DESIGN.md section 9 "Fused INT8 blocks" (unchanged from block_i8.hip); the image, the quantizer and a
// wave's conv are block_i8_core.h's, the weights pack_lconv_i8's (lconv_i8.h).
//
// A workgroup of four waves owns one position through a whole btl block, and two workgroups share a CU: one's staging
// and epilogues lie under the other's MFMAs.  LDS holds one zero-bordered 21 x 21 int8 image of 128 channels
// ([16-channel group][441 points][16], 56,448 B), which the block's tensors take in turn:
//   stage    x (fp16, 128 channels) -> q(mish(bn0(x))) into the whole image
//   reduce   1x1, K = 128 over it; after a barrier its quantizing epilogue writes image A over channels 0..63
//   inner j  3x3, K = 64 from A or B (B over channels 64..127); the quantizing epilogue writes the other one
//   expand   1x1, K = 64 from the last image, two passes of 64 output channels; + x, stored as fp16
// Wave w takes all 64 output channels of a pass (four 16-channel tiles) and the 16-point tiles w + 4 i of the 23 that
// cover the board: 96 accumulator registers.  Per tap and 64-channel K slice it reads four weight fragments from
// global memory (shared by the CU's eight waves through L1, the next step's prefetched under the MFMAs) and six
// activation fragments from LDS, and issues 24 MFMAs.
#include "block_i8.h"
#include "block_i8_core.h"

namespace p3 {

namespace {

using namespace i8blk;

constexpr int kWgC128 = 256;
constexpr int kLdsC128 = 8 * kGroupBytes;   // 128 channels: 56,448
static_assert(kLdsC128 <= 64 * 1024, "a static LDS array: the size is in the kernel's metadata");
static_assert(2 * kLdsC128 <= 160 * 1024 && kLdsC128 <= 81920, "two workgroups within the CU's 160 KiB of LDS");

template <int C, int CB, int L>
__global__ void __launch_bounds__(kWgC128, 2) k_block_i8(BlockI8Args a) {
  static_assert(C == 128 && CB == 64, "one 64-channel output pass per bottleneck conv, two for the expand");
  static_assert(L >= 1 && L + 2 <= kBlockI8MaxConvs, "one to three inner layers");
  constexpr int kImgB = (CB / 16) * kGroupBytes;   // a C_b-channel image: 28,224
  constexpr int kStageItems = (C / 16) * kNLoc;    // 2,888 sixteen-byte points of a position
  __shared__ __attribute__((aligned(16))) char smem[kLdsC128];
  const int tid = threadIdx.x, lane = tid & 63, pg = tid >> 6, g = lane >> 4;

  // the border of the image stays zero (only interior points are ever written)
  for (int i = tid; i < kLdsC128 / 16; i += kWgC128) *(i32x4*)(smem + 16 * i) = i32x4{0, 0, 0, 0};

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
      const int c0 = ct * 16 + 4 * g;
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

  __syncthreads();   // zeroed image before the first staged store
#pragma unroll 1
  for (int pos = blockIdx.x; pos < a.npos; pos += gridDim.x) {
    _Float16* x = a.x + (size_t)pos * C * kNLoc;
    // ---- stage q(mish(bn0(x))): 128 channels ---------------------------------------------------------------------
    {
      const float s0 = a.act_scale[a.q0];
#pragma unroll 2
      for (int it = tid; it < kStageItems; it += kWgC128) {
        const int gc = it / kNLoc, p = it - gc * kNLoc;
        const h8 lo = *(const h8*)(x + ((size_t)(2 * gc) * kNLoc + p) * 8);
        const h8 hi = *(const h8*)(x + ((size_t)(2 * gc + 1) * kNLoc + p) * 8);
        *(i32x4*)(smem + gc * kGroupBytes + pad_index(p) * 16) = stage_pre(lo, hi, a.scale[0], a.shift[0], gc * 16, s0);
      }
    }
    __syncthreads();
    // ---- reduce 1x1, 128 -> 64 ----------------------------------------------------------------------------------
    acc_zero();
    conv_i8<1, C / 64>(acc, smem, a.w[0] + lane * 16, pidx, ntile);
    __syncthreads();   // every wave has read the staged image: image A (channels 0..63 of it) is free
    store_q(0, a.act_scale[a.q0], a.act_scale[a.q0 + 1], smem);
    __syncthreads();
    // ---- inner 3x3 layers, ping-pong between A and B -----------------------------------------------------------
    int cur = 0;
#pragma unroll
    for (int j = 1; j <= L; ++j) {
      acc_zero();
      conv_i8<3, CB / 64>(acc, smem + cur * kImgB, a.w[j] + lane * 16, pidx, ntile);
      store_q(j, a.act_scale[a.q0 + j], a.act_scale[a.q0 + j + 1], smem + (1 - cur) * kImgB);
      __syncthreads();
      cur = 1 - cur;
    }
    // ---- expand 1x1, 64 -> 128, + x -----------------------------------------------------------------------------
    const float s_in = a.act_scale[a.q0 + L + 1];
#pragma unroll 1
    for (int cp = 0; cp < C / 64; ++cp) {
      acc_zero();
      conv_i8<1, CB / 64>(acc, smem + cur * kImgB, a.w[L + 1] + (size_t)cp * (CB / 64) * 4096 + lane * 16, pidx, ntile);
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
    __syncthreads();   // the image is free for the next position
  }
}

template <int L>
hipError_t launch_t(const BlockI8Args& a, int n_cu, hipStream_t s) {
  const int grid = a.npos < 2 * n_cu ? a.npos : 2 * n_cu;   // two workgroups per CU
  hipLaunchKernelGGL((k_block_i8<128, 64, L>), dim3(grid), dim3(kWgC128), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_block_i8_c128(const BlockI8Args& a, int n_cu, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  if (a.inner == 1) return launch_t<1>(a, n_cu, s);
  if (a.inner == 2) return launch_t<2>(a, n_cu, s);
  if (a.inner == 3) return launch_t<3>(a, n_cu, s);
  return hipErrorInvalidValue;
}

const char* block_i8_c128_kernel_name() { return "k_block_i8<128,64>"; }

}  // namespace p3
