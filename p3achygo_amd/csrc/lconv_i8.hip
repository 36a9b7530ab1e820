// lconv_i8.hip — the INT8 layer convs of the layer-wise trunks (P3HIP_FLAG_INT8) and the absmax reduction that
// calibrates their activation scales.  Numerics: DESIGN.md section 9.
//
// k_lconv_i8 runs one conv of a layer-wise block on v_mfma_i32_16x16x64_i8.  Operand layout:
//   activations  int8 [pos][C / 16][361][16]   (the fp16 path's [pos][C / 8][361][8] with 16 channels per 16-byte point)
//   weights      int8 [cout pass][K slice][tap][cout tile][64 lanes][16]  (lconv_i8.h pack_lconv_i8)
// MFMA lane map (checked on the GPU with exact asymmetric integer data): lane l holds A[row l & 15]
// [k = 16 (l >> 4) + j] and B[k = 16 (l >> 4) + j][col l & 15], j = 0..15, and D[row 4 (l >> 4) + r][col l & 15] in
// register r.  A = weights (row = output channel), B = activations (column = board point).
//
// A workgroup of four waves owns one position and one pass of 64 output channels.  Input channels are staged in
// 64-channel slices into a zero-bordered 21 x 21 LDS image (double-buffered: the next slice's global loads are in
// flight while the current one runs).  Wave w takes the 16-point tiles w, w + 4, .. of the 23 that cover the board
// and all four 16-channel output tiles: per tap it reads four weight fragments from global (shared by the workgroup's
// waves through L1) and six activation fragments from LDS, and issues 24 MFMAs.
#include "lconv_i8.h"
#include "conv_core.h"

namespace p3 {

typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kPad = 21;                       // padded board side
constexpr int kPadPts = kPad * kPad;           // 441
constexpr int kSliceCh = 64;                   // input channels per K slice
constexpr int kSliceBytes = (kSliceCh / 16) * kPadPts * 16;   // 28,224
constexpr int kWgI8 = 256;
constexpr int kStageItems = (kSliceCh / 16) * kNLoc;          // 1,444 sixteen-byte points per slice
constexpr int kStagePerThread = (kStageItems + kWgI8 - 1) / kWgI8; // 6
constexpr int kTiles = (kNLoc + 15) / 16;                      // 23 point tiles
constexpr int kTilesPerWave = (kTiles + 3) / 4;                // 6

__device__ __forceinline__ int pad_index(int loc) { return (loc / 19 + 1) * kPad + loc % 19 + 1; }

// q = clamp(rint(y / s), -127, 127); a zero scale (an all-zero tensor) quantizes everything to 0
__device__ __forceinline__ unsigned q8(float y, float s) {
  if (!(s > 0.0f)) return 0u;
  float q = __builtin_rintf(y / s);
  q = fminf(fmaxf(q, -127.0f), 127.0f);
  return (unsigned)((int)q) & 0xffu;
}

// PRE staging: 16 channels of one point from the raw fp16 stream, mish(bn(.)) and quantized
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

template <int KW, int CIN, int COUT, bool PRE, bool ACT, bool RES, bool DUAL>
__global__ void __launch_bounds__(kWgI8, 2) k_lconv_i8(LConvI8Args a) {
  static_assert(!(ACT && (RES || DUAL)), "act stores the activated tensor only");
  static_assert(CIN % kSliceCh == 0 && COUT % 64 == 0, "64-channel slices and passes");
  constexpr int NS = CIN / kSliceCh, NCP = COUT / 64, KK = KW * KW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cp = blockIdx.x % NCP;
  const int pos = blockIdx.x / NCP;
  if (pos >= a.npos) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4;

  // the border of both images stays zero (only interior points are ever staged)
  for (int i = tid; i < 2 * kSliceBytes / 16; i += kWgI8) *(i32x4*)(smem + 16 * i) = i32x4{0, 0, 0, 0};

  const float s_in = a.act_scale[a.in_scale];
  // staging: slice s -> registers -> LDS image
  i32x4 st[kStagePerThread];
  h8 pr[PRE ? 2 * kStagePerThread : 1];
  auto stage_load = [&](int s) {
#pragma unroll
    for (int k = 0; k < kStagePerThread; ++k) {
      int it = tid + kWgI8 * k;
      if (it >= kStageItems) it = kStageItems - 1;   // tail threads re-read a valid point (not stored)
      const int gc = it / kNLoc, p = it - gc * kNLoc, c16 = s * (kSliceCh / 16) + gc;
      if (PRE) {
        const _Float16* x = (const _Float16*)a.in + ((size_t)pos * (CIN / 8) + 2 * c16) * kNLoc * 8;
        pr[2 * k] = *(const h8*)(x + p * 8);
        pr[2 * k + 1] = *(const h8*)(x + kNLoc * 8 + p * 8);
      } else {
        st[k] = *(const i32x4*)((const int8_t*)a.in + (((size_t)pos * (CIN / 16) + c16) * kNLoc + p) * 16);
      }
    }
  };
  auto stage_store = [&](int s, char* img) {
#pragma unroll
    for (int k = 0; k < kStagePerThread; ++k) {
      const int it = tid + kWgI8 * k;
      if (it >= kStageItems) continue;
      const int gc = it / kNLoc, p = it - gc * kNLoc;
      i32x4 v;
      if (PRE) v = stage_pre(pr[2 * k], pr[2 * k + 1], a.scale_in, a.shift_in, (s * (kSliceCh / 16) + gc) * 16, s_in);
      else v = st[k];
      *(i32x4*)(img + (gc * kPadPts + pad_index(p)) * 16) = v;
    }
  };

  // this lane's board points: tile t = wid + 4 i, point 16 t + (lane & 15); points past the board read the image at
  // point 0's place (any in-range address) and are never stored
  int pidx[kTilesPerWave];
#pragma unroll
  for (int i = 0; i < kTilesPerWave; ++i) {
    const int loc = 16 * (wid + 4 * i) + (lane & 15);
    pidx[i] = (g * kPadPts + (loc < kNLoc ? pad_index(loc) : pad_index(0))) * 16;
  }
  const int ntile = wid + 4 * (kTilesPerWave - 1) < kTiles ? kTilesPerWave : kTilesPerWave - 1;   // wave-uniform

  i32x4 acc[kTilesPerWave][4];
#pragma unroll
  for (int i = 0; i < kTilesPerWave; ++i)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[i][ct] = i32x4{0, 0, 0, 0};

  __syncthreads();   // zeroed images before the first staged store
  stage_load(0);
  stage_store(0, smem);
  __syncthreads();
  const int8_t* wp = (const int8_t*)a.w + (size_t)cp * NS * KK * 4 * 1024 + lane * 16;
#pragma unroll 1
  for (int s = 0; s < NS; ++s) {
    if (s + 1 < NS) stage_load(s + 1);
    const char* img = smem + (s & 1) * kSliceBytes;
#pragma unroll 1
    for (int tap = 0; tap < KK; ++tap) {
      i32x4 A[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) A[ct] = *(const i32x4*)(wp + ((size_t)(s * KK + tap) * 4 + ct) * 1024);
      const int off = KW == 3 ? ((tap / 3 - 1) * kPad + (tap % 3 - 1)) * 16 : 0;
#pragma unroll
      for (int i = 0; i < kTilesPerWave; ++i) {
        if (i < ntile) {
          const i32x4 B = *(const i32x4*)(img + pidx[i] + off);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) acc[i][ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[ct], B, acc[i][ct], 0, 0, 0);
        }
      }
    }
    if (s + 1 < NS) stage_store(s + 1, smem + ((s + 1) & 1) * kSliceBytes);
    __syncthreads();
  }

  // epilogue: lane holds output channels c0 + r (r = 0..3) of board point loc, for every (tile, cout tile)
  const float s_out = (ACT || DUAL) ? a.act_scale[a.out_scale] : 0.0f;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int c0 = cp * 64 + ct * 16 + 4 * g;
    const f32x4 sw = *(const f32x4*)(a.w_scale + c0);
    f32x4 mult, sc = {0, 0, 0, 0}, sh = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) mult[r] = s_in * sw[r];
    if (ACT || DUAL) {
      sc = *(const f32x4*)(a.scale_out + c0);
      sh = *(const f32x4*)(a.shift_out + c0);
    }
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
      const int loc = 16 * (wid + 4 * i) + (lane & 15);
      if (i >= ntile || loc >= kNLoc) continue;
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (float)acc[i][ct][r] * mult[r];
      const size_t o16 = (((size_t)pos * (COUT / 8) + (c0 >> 3)) * kNLoc + loc) * 8 + (c0 & 7);     // fp16 layout
      const size_t o8 = (((size_t)pos * (COUT / 16) + (c0 >> 4)) * kNLoc + loc) * 16 + (c0 & 15);   // int8 layout
      if (RES) {
        const h4 old = *(const h4*)((const _Float16*)a.out + o16);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)old[r];
      }
      if (ACT || DUAL) {
        unsigned u = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) u |= q8(mish_f(v[r] * sc[r] + sh[r]), s_out) << (8 * r);
        *(unsigned*)((int8_t*)(ACT ? a.out : a.out2) + o8) = u;
      }
      if (!ACT) *(h4*)((_Float16*)a.out + o16) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    }
  }
}

// Largest |v| of an fp16 tensor [npos][C / 8][361][8], v = the stored value or mish(bn(value)), folded into *amax as
// float bits by an integer atomicMax (all candidates are >= 0, so the result does not depend on the order)
__global__ void __launch_bounds__(kWgI8) k_absmax(AbsmaxArgs a) {
  const size_t n = (size_t)a.npos * (a.C / 8) * kNLoc;
  float m = 0.0f;
  for (size_t i = (size_t)blockIdx.x * kWgI8 + threadIdx.x; i < n; i += (size_t)gridDim.x * kWgI8) {
    const h8 v = *(const h8*)(a.in + i * 8);
    const int c0 = (int)((i / kNLoc) % (a.C / 8)) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = (float)v[j];
      if (a.scale) x = mish_f(x * a.scale[c0 + j] + a.shift[c0 + j]);
      m = fmaxf(m, fabsf(x));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  if ((threadIdx.x & 63) == 0) atomicMax(a.amax, __float_as_uint(m));
}

}  // namespace

template <int KW, int CIN, int COUT, bool PRE, bool ACT, bool RES, bool DUAL>
static hipError_t launch_t(const LConvI8Args& a, hipStream_t s) {
  constexpr size_t lds = 2 * kSliceBytes;
  static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
  hipLaunchKernelGGL((k_lconv_i8<KW, CIN, COUT, PRE, ACT, RES, DUAL>), dim3(a.npos * (COUT / 64)), dim3(kWgI8), lds, s, a);
  return hipGetLastError();
}

// the ten layer shapes and flag sets launch_lconv dispatches (kernels.hip)
hipError_t launch_lconv_i8(int kw, int cin, int cout, const LConvI8Args& a, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  const int f = (a.pre ? 8 : 0) | (a.act ? 4 : 0) | (a.res ? 2 : 0) | (a.dual ? 1 : 0);
#define P3_LCONV_I8(KW, CIN, COUT, PRE, ACT, RES, DUAL) \
  if (kw == KW && cin == CIN && cout == COUT && f == ((PRE ? 8 : 0) | (ACT ? 4 : 0) | (RES ? 2 : 0) | (DUAL ? 1 : 0))) \
    return launch_t<KW, CIN, COUT, PRE, ACT, RES, DUAL>(a, s);
  P3_LCONV_I8(1, 384, 192, true, true, false, false)     // btl reduce from the raw stream
  P3_LCONV_I8(1, 384, 192, false, true, false, false)    // btl reduce from the activated copy
  P3_LCONV_I8(1, 384, 192, true, false, false, true)     // nbt reduce (t raw + act1(t))
  P3_LCONV_I8(1, 384, 192, false, false, false, true)
  P3_LCONV_I8(3, 192, 192, false, true, false, false)    // inner conv, activated output
  P3_LCONV_I8(3, 192, 192, true, true, false, false)     // classic conv0 from the raw stream
  P3_LCONV_I8(3, 192, 192, false, false, true, false)    // classic conv1 (+x), last block
  P3_LCONV_I8(3, 192, 192, false, false, true, true)     // nbt conv2 / conv4, classic conv1 (+x, + next act)
  P3_LCONV_I8(1, 192, 384, false, false, true, false)    // expand + x
  P3_LCONV_I8(1, 192, 384, false, false, true, true)     // expand + x, + the next block's activated input
#undef P3_LCONV_I8
  return hipErrorInvalidValue;
}

const char* lconv_i8_kernel_name(int kw, int cin, int cout) {
  if (kw == 3 && cin == 192 && cout == 192) return "k_lconv_i8<3,192,192>";
  if (kw == 1 && cin == 384) return "k_lconv_i8<1,384,192>";
  if (kw == 1 && cin == 192) return "k_lconv_i8<1,192,384>";
  return "k_lconv_i8";
}

hipError_t launch_absmax(const AbsmaxArgs& a, int n_cu, hipStream_t s) {
  if (a.npos < 1) return hipSuccess;
  const size_t n = (size_t)a.npos * (a.C / 8) * kNLoc;
  size_t grid = (n + kWgI8 - 1) / kWgI8;
  if (grid > (size_t)4 * n_cu) grid = (size_t)4 * n_cu;
  hipLaunchKernelGGL(k_absmax, dim3((unsigned)grid), dim3(kWgI8), 0, s, a);
  return hipGetLastError();
}

}  // namespace p3
