// block_i8.hip — the fused INT8 block kernel of the btl trunks, written once for both widths: geometry <256,128>
// (C = 256 / C_b = 128, P3HIP_FLAG_INT8_FUSED) and geometry <128,64> (C = 128 / C_b = 64, P3HIP_FLAG_INT8_C128).
// Numerics: DESIGN.md section 9 "Fused INT8 blocks"; operand layouts and the lane map of v_mfma_i32_16x16x64_i8 are those
// of lconv_i8.hip (weights in pack_lconv_i8 order, lconv_i8.h).
//
// A workgroup owns one position through a whole btl block; the activations never leave the chip between the block's
// convs.  LDS holds one zero-bordered 21 x 21 int8 image of C channels ([16-channel group][441 points][16]), which is
// also two images of C_b channels each, and the block's tensors take them in turn:
//   stage    x (fp16, C channels) -> q(mish(bn0(x))) into the whole LDS (both images), once
//   reduce   1x1, K = C over both images; after a barrier its quantizing epilogue writes image 0
//   inner j  3x3, K = C_b from image cur; the quantizing epilogue writes image 1 - cur
//   expand   1x1, K = C_b from image cur, in passes of 64 output channels, two per wave; + x, stored as fp16
// The input of a layer is staged once, not once per 64-channel output pass.  A wave takes 64 output channels (four
// 16-channel tiles) and the 16-point tiles pg + 4 i of the 23 that cover the board: 96 accumulator registers.  Per tap
// and 64-channel K slice it reads four weight fragments from global memory (shared by the CU's eight waves through L1,
// the next step's prefetched under the MFMAs) and six activation fragments from LDS, and issues 24 MFMAs.
//   <256,128>  eight waves: wave w has channel half w & 1 (64 of the 128 bottleneck channels) and pg = w >> 1.  The
//              images are 56,448 B each, 112,896 B together: dynamic LDS, one workgroup per CU.
//   <128,64>   four waves: every wave has all 64 bottleneck channels, pg = w.  The images are 28,224 B each, 56,448 B
//              together: a static array, and two workgroups share a CU, one's staging and epilogues under the other's
//              MFMAs.
#include <stdint.h>

#include "block_i8.h"
#include "conv_core.h"
#include "launch_util.h"

namespace p3 {

typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

struct G256 { static constexpr int C = 256, CB = 128, kWaves = 8, kWgPerCu = 1; };
struct G128 { static constexpr int C = 128, CB = 64, kWaves = 4, kWgPerCu = 2; };

constexpr int kPad = 21;                        // padded board side
constexpr int kPadPts = kPad * kPad;            // 441
constexpr int kGroupBytes = kPadPts * 16;       // 16 channels of the padded board: 7,056
constexpr int kSliceBytes = 4 * kGroupBytes;    // a 64-channel K slice: 28,224
constexpr int kTiles = (kNLoc + 15) / 16;       // 23 point tiles
constexpr int kTilesPerWave = (kTiles + 3) / 4; // 6
constexpr int kStaticLdsMax = 64 * 1024;        // up to here a static array, its size in the kernel's metadata

__device__ __forceinline__ int pad_index(int loc) { return (loc / 19 + 1) * kPad + loc % 19 + 1; }

// q = clamp(rint(y / s), -127, 127); a zero scale (an all-zero tensor) quantizes everything to 0
__device__ __forceinline__ unsigned q8(float y, float s) {
  if (!(s > 0.0f)) return 0u;
  float q = __builtin_rintf(y / s);
  q = fminf(fmaxf(q, -127.0f), 127.0f);
  return (unsigned)((int)q) & 0xffu;
}

// 16 channels of one point from the raw fp16 stream, mish(bn0(.)) and quantized
__device__ __forceinline__ i32x4 stage_pre(const h8& lo, const h8& hi, const float* sc, const float* sh, int c0, float s) {
  i32x4 r;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    unsigned u = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = 4 * w + b, c = c0 + j;
      const float x = (float)(j < 8 ? lo[j] : hi[j - 8]);
      u |= q8(mish_f(x * sc[c] + sh[c]), s) << (8 * b);
    }
    r[w] = (int)u;
  }
  return r;
}

// acc[i][ct] += W . a over NS 64-channel K slices of the image(s) at `img` and the KW x KW taps.  wp: this wave's
// output pass of the conv's weight stream plus lane * 16; the (slice, tap) steps lie 4 KB apart in it.
template <int KW, int NS>
__device__ __forceinline__ void conv_i8(i32x4 (&acc)[kTilesPerWave][4], const char* img, const int8_t* wp,
                                        const int (&pidx)[kTilesPerWave], int ntile) {
  constexpr int KK = KW * KW, NT = NS * KK;
  i32x4 A[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) A[ct] = *(const i32x4*)(wp + ct * 1024);
#pragma unroll 1
  for (int t = 0; t < NT; ++t) {
    const int tn = t + 1 < NT ? t + 1 : t;   // the last step re-reads its own fragments
    i32x4 An[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) An[ct] = *(const i32x4*)(wp + ((size_t)tn * 4 + ct) * 1024);
    const int s = t / KK, tap = t - s * KK;
    const int off = s * kSliceBytes + (KW == 3 ? ((tap / 3 - 1) * kPad + (tap % 3 - 1)) * 16 : 0);
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
      if (i < ntile) {
        const i32x4 B = *(const i32x4*)(img + pidx[i] + off);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[i][ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[ct], B, acc[i][ct], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) A[ct] = An[ct];
  }
}

// the workgroup's LDS: a static array where it fits one, dynamic LDS (ensure_lds at launch) otherwise
template <int kBytes>
__device__ __forceinline__ char* lds_images() {
  if constexpr (kBytes <= kStaticLdsMax) {
    __shared__ __attribute__((aligned(16))) char smem[kBytes];
    return smem;
  } else {
    extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
    return smem_dyn;
  }
}

template <class G, int L>
__global__ void __launch_bounds__(64 * G::kWaves, G::kWgPerCu) k_block_i8(BlockI8Args a) {
  constexpr int C = G::C, CB = G::CB, kWg = 64 * G::kWaves;
  constexpr int kHalves = G::kWaves / 4;            // 64-channel halves of C_b, one per wave of a point group
  constexpr int kImgB = (CB / 16) * kGroupBytes;    // a C_b-channel image
  constexpr int kLdsBytes = (C / 16) * kGroupBytes; // the staged x: both images
  constexpr int kStageItems = (C / 16) * kNLoc;     // sixteen-byte points of a position
  static_assert(C == 2 * CB && CB == 64 * kHalves, "one 64-channel output pass per wave and bottleneck conv, two for the expand");
  static_assert(G::kWgPerCu * kLdsBytes <= 160 * 1024, "the CU's workgroups within its 160 KiB of LDS");
  static_assert(L >= 1 && L + 2 <= kBlockI8MaxConvs, "one to three inner layers");
  char* const smem = lds_images<kLdsBytes>();
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4;
  const int half = wid % kHalves, pg = wid / kHalves;

  // the border of both images stays zero (only interior points are ever written)
  for (int i = tid; i < kLdsBytes / 16; i += kWg) *(i32x4*)(smem + 16 * i) = i32x4{0, 0, 0, 0};

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
    _Float16* x = a.x + (size_t)pos * C * kNLoc;
    // ---- stage q(mish(bn0(x))): C channels into both images ---------------------------------------------------
    {
      const float s0 = a.act_scale[a.q0];
#pragma unroll 2
      for (int it = tid; it < kStageItems; it += kWg) {
        const int gc = it / kNLoc, p = it - gc * kNLoc;
        const h8 lo = *(const h8*)(x + ((size_t)(2 * gc) * kNLoc + p) * 8);
        const h8 hi = *(const h8*)(x + ((size_t)(2 * gc + 1) * kNLoc + p) * 8);
        *(i32x4*)(smem + gc * kGroupBytes + pad_index(p) * 16) = stage_pre(lo, hi, a.scale[0], a.shift[0], gc * 16, s0);
      }
    }
    __syncthreads();
    // ---- reduce 1x1, C -> C_b -----------------------------------------------------------------------------------
    acc_zero();
    conv_i8<1, C / 64>(acc, smem, a.w[0] + (size_t)half * (C / 64) * 4096 + lane * 16, pidx, ntile);
    __syncthreads();   // every wave has read both images: image 0 is free
    store_q(0, a.act_scale[a.q0], a.act_scale[a.q0 + 1], smem);
    __syncthreads();
    // ---- inner 3x3 layers, ping-pong between the images --------------------------------------------------------
    int cur = 0;
#pragma unroll
    for (int j = 1; j <= L; ++j) {
      acc_zero();
      conv_i8<3, CB / 64>(acc, smem + cur * kImgB, a.w[j] + (size_t)half * (CB / 64) * 9 * 4096 + lane * 16, pidx, ntile);
      store_q(j, a.act_scale[a.q0 + j], a.act_scale[a.q0 + j + 1], smem + (1 - cur) * kImgB);
      __syncthreads();
      cur = 1 - cur;
    }
    // ---- expand 1x1, C_b -> C, + x ------------------------------------------------------------------------------
    const float s_in = a.act_scale[a.q0 + L + 1];
#pragma unroll 1
    for (int k = 0; k < (C / 64) / kHalves; ++k) {
      const int cp = half + kHalves * k;
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
    __syncthreads();   // the images are free for the next position
  }
}

template <class G, int L>
hipError_t launch_t(const BlockI8Args& a, int n_cu, hipStream_t s) {
  constexpr int kLdsBytes = (G::C / 16) * kGroupBytes;
  constexpr int kDynLds = kLdsBytes <= kStaticLdsMax ? 0 : kLdsBytes;   // a static-LDS geometry passes 0 dynamic bytes
  if constexpr (kDynLds > 0) {
    static AttrOnce once;   // dynamic LDS above 64 KB needs the attribute, once per kernel and device
    if (hipError_t e = ensure_lds(once, k_block_i8<G, L>, kDynLds); e != hipSuccess) return e;
  }
  const int grid = a.npos < G::kWgPerCu * n_cu ? a.npos : G::kWgPerCu * n_cu;
  hipLaunchKernelGGL((k_block_i8<G, L>), dim3(grid), dim3(64 * G::kWaves), kDynLds, s, a);
  return hipGetLastError();
}

template <class G>
hipError_t launch_g(const BlockI8Args& a, int n_cu, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  if (a.inner == 1) return launch_t<G, 1>(a, n_cu, s);
  if (a.inner == 2) return launch_t<G, 2>(a, n_cu, s);
  if (a.inner == 3) return launch_t<G, 3>(a, n_cu, s);
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_block_i8(int C, const BlockI8Args& a, int n_cu, hipStream_t s) {
  if (C == G256::C) return launch_g<G256>(a, n_cu, s);
  if (C == G128::C) return launch_g<G128>(a, n_cu, s);
  return hipErrorInvalidValue;
}

const char* block_i8_kernel_name(int C) {
  return C == G256::C ? "k_block_i8<256,128>" : C == G128::C ? "k_block_i8<128,64>" : nullptr;
}

}  // namespace p3
