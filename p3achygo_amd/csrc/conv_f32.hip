// conv_f32.hip — gfx950 kernels of the fp32 plan of the conv trunks (conv_f32.h, P3HIP_FLAG_FP32).
//
// Every conv is a GEMM per position, out[cout][point] = sum over (tap, cin) W[tap][cin][cout] * in[cin][point + tap], on
// v_mfma_f32_32x32x2_f32: the weights are the A operand (rows = 32 output channels), the activations the B operand
// (columns = 32 board points), and a lane's 16 accumulators are four channel quads of one board point — the 16-byte
// pieces of the [C / 8][361][8] layout.  A workgroup of four waves computes 64 output channels of one position; a wave
// owns every fourth tile of 32 board points and keeps its sums in registers across the K slices.
//
// LDS holds one K slice of 32 input channels as four planes of 8 channels, [group][slot][8] floats, where a slot is a
// point of the zero-padded board: slot = PADTOP + y * S + x with S = 19 + KW / 2, so that the pad columns between two
// rows serve both, and PADTOP slots above and below.  Only board points are ever written; the padding is zeroed once.
// Output rows r = y * S + x run over the same grid (x >= 19 and y >= 19 are computed and dropped), so the B operand of
// tap (ky, kx) is the slot r + PADTOP + (ky - KW / 2) * S + (kx - KW / 2): one ds_read_b128 per lane gives the four
// k-steps of a channel group (lane half h owns channels 4 h .. 4 h + 3), 64 lanes read 1 KB without a bank conflict.
//
// The weights come straight from global memory as packed fragments (pack_conv_f32), one 16-byte load per lane and
// fragment, fetched one step ahead of the MFMAs that use them: all positions share them and they stay in L2.
// Activation offsets are 64-bit per position; the 32-bit offsets stay inside one position's C x 361 floats.
#include "conv_f32.h"

#include <hip/hip_runtime.h>

#include "conv_core.h"   // mish_f, f32x4, f32x16
#include "layer_kernels.h"   // FeatOff

namespace p3 {

namespace {

constexpr int kPosFloats = kNLoc * 8;   // one channel group of one position

template <int KW>
struct GeoF {
  static constexpr int PAD = KW / 2, S = kBL + PAD, PADTOP = PAD * S + PAD;
  static constexpr int NROWS = (kBL - 1) * S + kBL;
  static constexpr int NTILES = (NROWS + 31) / 32;   // tiles of 32 output rows
  static constexpr int NT = (NTILES + 3) / 4;        // per wave
  static constexpr int NSLOT = PADTOP + NTILES * 32 + PADTOP;
  static constexpr int PLANE = NSLOT * 32;           // bytes of one 8-channel plane
};

__device__ __forceinline__ void lds_zero(char* smem, int bytes) {
  for (int i = threadIdx.x * 16; i < bytes; i += blockDim.x * 16) *(f32x4*)(smem + i) = f32x4{0, 0, 0, 0};
}

// NG channel groups of the slice in LDS against the weight fragments of channel groups gg0 .. gg0 + NG of `wp`, the
// image of this output pass ([tap][ngtot groups][2 cout tiles][64 lanes][4]); every tap, accumulated into acc.
template <int KW, int NG>
__device__ __forceinline__ void conv_slice(const char* smem, const float* __restrict__ wp, int ngtot, int gg0,
                                           f32x16 (&acc)[2][GeoF<KW>::NT]) {
  using G = GeoF<KW>;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const f32x4* wf = (const f32x4*)wp + lane;
  auto frag = [&](int tap, int g) { return (size_t)((tap * ngtot + gg0 + g) * 2) * 64; };
  f32x4 a0 = wf[frag(0, 0)], a1 = wf[frag(0, 0) + 64];
  const char* bbase = smem + (G::PADTOP + wave * 32 + (lane & 31)) * 32 + (lane >> 5) * 16;
#pragma unroll 1
  for (int tap = 0; tap < KW * KW; ++tap) {
    const int ky = tap / KW, kx = tap - ky * KW;
    const int off = ((ky - G::PAD) * G::S + (kx - G::PAD)) * 32;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      // the next step's fragments (the last step re-reads its own)
      const int ntap = g + 1 < NG ? tap : (tap + 1 < KW * KW ? tap + 1 : tap);
      const int ng = g + 1 < NG ? g + 1 : (tap + 1 < KW * KW ? 0 : g);
      const f32x4 n0 = wf[frag(ntap, ng)], n1 = wf[frag(ntap, ng) + 64];
      f32x4 b[G::NT];
#pragma unroll
      for (int j = 0; j < G::NT; ++j) {
        b[j] = f32x4{0, 0, 0, 0};
        if (G::NTILES % 4 == 0 || wave + 4 * j < G::NTILES) b[j] = *(const f32x4*)(bbase + g * G::PLANE + j * 4096 + off);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < G::NT; ++j) {
          if (G::NTILES % 4 != 0 && wave + 4 * j >= G::NTILES) continue;
          acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b[j][s], acc[0][j], 0, 0, 0);
          acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b[j][s], acc[1][j], 0, 0, 0);
        }
      a0 = n0;
      a1 = n1;
    }
  }
}

template <int KW>
__device__ __forceinline__ void acc_clear(f32x16 (&acc)[2][GeoF<KW>::NT]) {
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int j = 0; j < GeoF<KW>::NT; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][j][i] = 0.0f;
}

// the board point of output row r = 32 tile + (lane & 31); false for the padding rows
template <int KW>
__device__ __forceinline__ bool row_point(int r, int& loc) {
  using G = GeoF<KW>;
  const int y = r / G::S, x = r - y * G::S;
  loc = y * kBL + x;
  return x < kBL && y < kBL;
}

}  // namespace

// =======================================================================================
// Stem: 5x5 conv over the 15 planes expanded from the feature record (a 16th plane of zeros makes two channel groups),
// plus the game-state dense.  One (position, 64 output channels) item per workgroup turn.
// =======================================================================================
__global__ void __launch_bounds__(256, 2) k_init_f32(InitF32Args a) {
  using G = GeoF<5>;
  __shared__ __attribute__((aligned(16))) char smem[2 * G::PLANE];
  __shared__ float bias_lds[64];
  lds_zero(smem, 2 * G::PLANE);
  __syncthreads();
  const int C = a.C, ncp = C / 64;
  const int items = a.npos * ncp;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 31, h = lane >> 5;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int pos = item / ncp, cp = item - pos * ncp;
    const unsigned char* f = (const unsigned char*)a.feats + (size_t)pos * FeatOff::size;
    const int color = (signed char)f[FeatOff::color];
    for (int loc = threadIdx.x; loc < kNLoc; loc += 256) {
      f32x4 p[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};   // planes 0 .. 15
      auto our = [&](int off) { return (signed char)f[off + loc] == color ? 1.0f : 0.0f; };
      auto opp = [&](int off) { return (signed char)f[off + loc] == -color ? 1.0f : 0.0f; };
      p[0][0] = our(FeatOff::board); p[0][1] = opp(FeatOff::board);
      p[1][3] = our(FeatOff::atari); p[2][0] = opp(FeatOff::atari);
      p[2][1] = our(FeatOff::two); p[2][2] = opp(FeatOff::two);
      p[2][3] = our(FeatOff::three); p[3][0] = opp(FeatOff::three);
      p[3][1] = our(FeatOff::ladder); p[3][2] = opp(FeatOff::ladder);
      const int y = loc / kBL, xx = loc - y * kBL;
      float lastm[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const int* lm = (const int*)(f + FeatOff::last + m * 8);
        lastm[m] = (lm[0] == y && lm[1] == xx) ? 1.0f : 0.0f;   // pass {19,0} / noop never match
      }
      p[0][2] = lastm[0]; p[0][3] = lastm[1]; p[1][0] = lastm[2]; p[1][1] = lastm[3]; p[1][2] = lastm[4];
      char* dst = smem + (G::PADTOP + y * G::S + xx) * 32;
      *(f32x4*)(dst) = p[0];
      *(f32x4*)(dst + 16) = p[1];
      *(f32x4*)(dst + G::PLANE) = p[2];
      *(f32x4*)(dst + G::PLANE + 16) = p[3];
    }
    if (threadIdx.x < 64) {
      float gsv[8];
      gsv[0] = color == 1 ? 1.0f : 0.0f;
      gsv[1] = color == 1 ? 0.0f : 1.0f;
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const int* lm = (const int*)(f + FeatOff::last + m * 8);
        gsv[2 + m] = (lm[0] == 19 && lm[1] == 0) ? 1.0f : 0.0f;
      }
      gsv[7] = (color == 1 ? -1.0f : 1.0f) * (*(const float*)(f + FeatOff::komi)) / 15.0f;
      const int c = cp * 64 + threadIdx.x;
      float b = a.game_b[c];
#pragma unroll
      for (int k = 0; k < 8; ++k) b += a.game_w[k * C + c] * gsv[k];
      bias_lds[threadIdx.x] = b;
    }
    __syncthreads();
    f32x16 acc[2][G::NT];
    acc_clear<5>(acc);
    conv_slice<5, 2>(smem, a.w + (size_t)cp * 25 * 16 * 64, 2, 0, acc);
#pragma unroll
    for (int j = 0; j < G::NT; ++j) {
      int loc;
      if (wave + 4 * j >= G::NTILES || !row_point<5>((wave + 4 * j) * 32 + lr, loc)) continue;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cl = mt * 32 + 8 * q + 4 * h;
          const f32x4 bias = *(const f32x4*)(bias_lds + cl);
          const f32x4 v = f32x4{acc[mt][j][4 * q], acc[mt][j][4 * q + 1], acc[mt][j][4 * q + 2], acc[mt][j][4 * q + 3]} + bias;
          *(f32x4*)(a.x + ((size_t)pos * (C / 8) + ((cp * 64 + cl) >> 3)) * kPosFloats + loc * 8 + 4 * h) = v;
        }
    }
    __syncthreads();   // the next item rewrites the planes and the bias
  }
}

// =======================================================================================
// Layer conv, kw 1 or 3, and the per-position 1x1 convs (LConvF32Args).  One (position, 64 output channels) item per
// workgroup turn, K slices of 32 input channels through LDS.
// =======================================================================================
template <int KW>
__global__ void __launch_bounds__(256, 2) k_lconv_f32(LConvF32Args a) {
  using G = GeoF<KW>;
  __shared__ __attribute__((aligned(16))) char smem[4 * G::PLANE];
  lds_zero(smem, 4 * G::PLANE);
  __syncthreads();
  const int ncp = a.cout / 64, ngtot = a.cin / 8, nslice = a.cin / 32;
  const int items = a.npos * ncp;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 31, h = lane >> 5;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int pos = item / ncp, cp = item - pos * ncp;
    const float* wp = a.w + (size_t)cp * (KW * KW) * a.cin * 64;
    const float* src = a.in + (size_t)pos * ngtot * kPosFloats;
    // Every K slice is summed on its own (a chain of 32 KW^2 products on the MFMA) and the slice sums are added up in
    // `tot`: the rounding error of an fp32 chain grows with its length, and one chain over a 3x3 conv of 512 channels
    // would be 4,608 products long.  Measured on a K = 1,728 conv against float64: 3.7 times the error in one chain.
    f32x16 tot[2][G::NT];
    acc_clear<KW>(tot);
#pragma unroll 1
    for (int sl = 0; sl < nslice; ++sl) {
      f32x16 acc[2][G::NT];
      acc_clear<KW>(acc);
      // stage channel groups 4 sl .. 4 sl + 3: 16-byte pieces idx = (group, point, half), contiguous in global memory
      for (int idx = threadIdx.x; idx < 4 * kNLoc * 2; idx += 256) {
        const int g = idx / (kNLoc * 2), rem = idx - g * (kNLoc * 2), loc = rem >> 1, hh = rem & 1;
        f32x4 v = *(const f32x4*)(src + (size_t)sl * 4 * kPosFloats + idx * 4);
        if (a.pre) {
          const int c = (sl * 4 + g) * 8 + hh * 4;
          const f32x4 sc = *(const f32x4*)(a.scale_in + c), sh = *(const f32x4*)(a.shift_in + c);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = mish_f(v[i] * sc[i] + sh[i]);
        }
        const int y = loc / kBL, xx = loc - y * kBL;
        *(f32x4*)(smem + g * G::PLANE + (G::PADTOP + y * G::S + xx) * 32 + hh * 16) = v;
      }
      __syncthreads();
      conv_slice<KW, 4>(smem, wp, ngtot, sl * 4, acc);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int j = 0; j < G::NT; ++j) tot[mt][j] += acc[mt][j];
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < G::NT; ++j) {
      int loc;
      if (!row_point<KW>((wave + 4 * j) * 32 + lr, loc)) continue;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = cp * 64 + mt * 32 + 8 * q + 4 * h;   // first channel of the quad
          f32x4 v = {tot[mt][j][4 * q], tot[mt][j][4 * q + 1], tot[mt][j][4 * q + 2], tot[mt][j][4 * q + 3]};
          if (a.hp) {
            if (c < 96) *(f32x4*)(a.out + (((size_t)pos * 24 + (c >> 2)) * kNLoc + loc) * 4) = v;
            continue;
          }
          const size_t o = ((size_t)pos * (a.cout / 8) + (c >> 3)) * kPosFloats + loc * 8 + 4 * h;
          if (a.res) v += *(const f32x4*)(a.out + o);
          if (a.dual) *(f32x4*)(a.out + o) = v;
          if (a.act == 1 || a.dual) {
            const f32x4 sc = *(const f32x4*)(a.scale_out + c), sh = *(const f32x4*)(a.shift_out + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = mish_f(v[i] * sc[i] + sh[i]);
          } else if (a.act == 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = mish_f(v[i]);
          }
          *(f32x4*)((a.dual ? a.out2 : a.out) + o) = v;
        }
    }
  }
}

// =======================================================================================
// Broadcast dense: u[c][j] = mish(bn1(sum_i t[c][i] W[i][j] + b[j])).  Here the activations are the A operand (rows =
// 32 channels, k = board point i) and the dense matrix the B operand (columns = 32 board points j), so that a lane again
// ends with channel quads of one point.  One (position, 32 channels) item per workgroup turn: t is transposed into LDS as
// [channel][i], rows of 368 + 4 floats with i >= 361 zeroed once (the packed matrix has zero rows there).
// =======================================================================================
namespace {
constexpr int kTtRow = 8 * kDenseF32Groups + 4;   // floats per channel row
}

__global__ void __launch_bounds__(256, 2) k_bdense_f32(BDenseF32Args a) {
  __shared__ __attribute__((aligned(16))) float tt[32 * kTtRow];
  lds_zero((char*)tt, 32 * kTtRow * 4);
  __syncthreads();
  const int C = a.C, nchunk = C / 32;
  const int items = a.npos * nchunk;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 31, h = lane >> 5;
  const f32x4* wf = (const f32x4*)a.w + lane;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int pos = item / nchunk, ch = item - pos * nchunk;
    const float* src = a.t + ((size_t)pos * (C / 8) + ch * 4) * kPosFloats;
    for (int idx = threadIdx.x; idx < 4 * kNLoc * 2; idx += 256) {
      const int g = idx / (kNLoc * 2), rem = idx - g * (kNLoc * 2), loc = rem >> 1, hh = rem & 1;
      const f32x4 v = *(const f32x4*)(src + idx * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) tt[(g * 8 + hh * 4 + i) * kTtRow + loc] = v[i];
    }
    __syncthreads();
    f32x16 acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
    auto frag = [&](int j, int g) { return (size_t)((wave + 4 * j) * kDenseF32Groups + g) * 64; };
    f32x4 b[3] = {wf[frag(0, 0)], wf[frag(1, 0)], wf[frag(2, 0)]};
#pragma unroll 2
    for (int g = 0; g < kDenseF32Groups; ++g) {
      const int ng = g + 1 < kDenseF32Groups ? g + 1 : g;
      const f32x4 n[3] = {wf[frag(0, ng)], wf[frag(1, ng)], wf[frag(2, ng)]};
      const f32x4 av = *(const f32x4*)(tt + lr * kTtRow + 8 * g + 4 * h);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], b[j][s], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 3; ++j) b[j] = n[j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int jj = (wave + 4 * j) * 32 + lr;
      if (jj >= kNLoc) continue;
      const float bj = a.bias[jj];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = ch * 32 + 8 * q + 4 * h;
        const f32x4 sc = *(const f32x4*)(a.scale + c), sh = *(const f32x4*)(a.shift + c);
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = mish_f((acc[j][4 * q + i] + bj) * sc[i] + sh[i]);
        *(f32x4*)(a.u + ((size_t)pos * (C / 8) + (c >> 3)) * kPosFloats + jj * 8 + 4 * h) = v;
      }
    }
    __syncthreads();   // the next item rewrites tt
  }
}

// =======================================================================================
// Host-side launchers
// =======================================================================================
namespace {

bool width_ok(int c) { return c >= 64 && c <= kF32MaxC && c % 64 == 0; }

// two workgroups per CU, one turn per (position, pass) item
int item_grid(long items, int n_cu) { return (int)(items < 2L * n_cu ? items : 2L * n_cu); }

}  // namespace

hipError_t launch_init_f32(const InitF32Args& a, int n_cu, hipStream_t s) {
  if (!width_ok(a.C) || a.npos < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_init_f32, dim3(item_grid((long)a.npos * (a.C / 64), n_cu)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_lconv_f32(int kw, const LConvF32Args& a, int n_cu, hipStream_t s) {
  if (!width_ok(a.cin) || !width_ok(a.cout) || a.npos < 1 || (kw != 1 && kw != 3)) return hipErrorInvalidValue;
  if (a.hp && (a.cout != 128 || kw != 1 || a.pre || a.act || a.res || a.dual)) return hipErrorInvalidValue;
  const int grid = item_grid((long)a.npos * (a.cout / 64), n_cu);
  if (kw == 3) hipLaunchKernelGGL(k_lconv_f32<3>, dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_lconv_f32<1>, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

const char* lconv_f32_kernel_name(int kw) { return kw == 3 ? "k_lconv_f32<3>" : "k_lconv_f32<1>"; }

hipError_t launch_bdense_f32(const BDenseF32Args& a, int n_cu, hipStream_t s) {
  if (!width_ok(a.C) || a.npos < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bdense_f32, dim3(item_grid((long)a.npos * (a.C / 32), n_cu)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace p3
