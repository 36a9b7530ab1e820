// conv_wino.hip — k_wconv, the 3x3 layer conv of the Winograd plan (conv_wino.h, P3HIP_FLAG_WINOGRAD), for gfx950.
//
// F(2x2, 3x3): Y = A^T [ sum over cin (G g G^T) . (B^T d B) ] A per tile and output channel, the sum over cin and the
// elementwise product of the 16 planes as 16 GEMMs M_p[cout][tile] = sum over cin U_p[cin][cout] V_p[cin][tile] on
// v_mfma_f32_16x16x32_f16: the weights U_p are the A operand (16 output channels x 32 input channels, read from the
// packed image straight into fragments), the transformed input V_p the B operand (32 input channels x 16 tiles, lane
// quarter q holds the 16-byte piece of channel group q), and a lane's four accumulators are four consecutive output
// channels of one tile.
//
// A unit of work is 32 flat tiles x 64 output channels (conv_wino.h wconv_unit).  Wave w of the workgroup owns the
// channel tile w of the unit and both tile blocks of 16: 16 planes x 2 blocks x 4 = 128 fp32 accumulators per lane (a
// unit of 64 tiles, 256 accumulators, left the allocator no room and spilled).  K runs in slices of 64 input channels,
// two MFMA steps of 32, slice by slice, step by step, every tile the same chain whatever unit it lands in.  Per slice,
// thread (tile ts = tid & 31, channel group g = tid >> 5) holds the tile's 4 x 4 patch of its 8 channels (fetched one
// slice ahead; activated with mish(bn_in(.)) and rounded to fp16 when PRE), takes V = B^T d B in two fp16 stages (each
// element a single fp16 add or subtract, so each rounds once) and stores the 16 planes to LDS, V[plane][group][tile][8]
// (64 KB): a wave's ds_read_b128 of a B fragment takes four runs of 256 bytes, 512 bytes apart, one per lane quarter,
// which are conflict-free.  The slice's 32 weight fragments go from the image (L2) straight to registers, the first 16
// before the barrier.  After the K loop the wave takes Y = A^T M A in fp32 in a fixed order and runs the layer's
// epilogue (res, BN, mish) on it.  Resources (tests/test_winograd_cpu.py reads them from the metadata): 411 - 415 unified
// registers, no scratch, 64 KB LDS: one wave per SIMD, one workgroup per CU.  Activation offsets are 64-bit per position.
#include "conv_wino.h"

#include <hip/hip_runtime.h>

#include "conv_core.h"   // mish_f, h8, h4, f32x4

namespace p3 {

namespace {

constexpr int kWWG = 256;
constexpr int kPosHalves = kNLoc * 8;   // one channel group of one position
constexpr int kVPlane = 8 * kWinoUnitTiles * 16;   // bytes of one plane of V: 8 channel groups x 32 tiles x 16
constexpr int kVBytes = 16 * kVPlane;

}  // namespace

template <bool PRE>
__global__ void __launch_bounds__(kWWG) k_wconv(WConvArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[kVBytes];
  const int lane = threadIdx.x & 63, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ts = threadIdx.x & 31, g = threadIdx.x >> 5;   // the staging role: tile of the unit, channel group of the K step
  const int nks = a.cin / 64;
  const long units = wconv_units(a.npos, a.cout);
  const long total = (long)a.npos * kWinoTiles;
  for (long unit = blockIdx.x; unit < units; unit += gridDim.x) {
    long tile0;
    int ntiles, cout0;
    wconv_unit(a.npos, a.cout, unit, &tile0, &ntiles, &cout0);
    // ---- this thread's patch: position, corner, and which of its 16 points lie on the board
    const bool tvalid = ts < ntiles;
    const long ft = tvalid ? tile0 + ts : total - 1;
    const int spos = (int)(ft / kWinoTiles), st = (int)(ft - (long)spos * kWinoTiles);
    const int y0 = 2 * (st / 10) - 1, x0 = 2 * (st % 10) - 1;
    unsigned onboard = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int y = y0 + (i >> 2), x = x0 + (i & 3);
      if (tvalid && y >= 0 && y < kBL && x >= 0 && x < kBL) onboard |= 1u << i;
    }
    // (a point off the board reads the position's first piece instead, and is zeroed: no address leaves the tensor)
    const _Float16* pbase = a.in + (size_t)spos * a.cin * kNLoc + (size_t)g * kPosHalves;
    const int corner = (y0 * kBL + x0) * 8;
    h8 d[16];
    auto patch_load = [&](int ks) {
      const _Float16* s = pbase + (size_t)ks * 8 * kPosHalves;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const bool on = onboard >> i & 1;
        const h8 v = *(const h8*)(s + (on ? corner + ((i >> 2) * kBL + (i & 3)) * 8 : 0));
        d[i] = on ? v : h8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    };
    patch_load(0);
    // the wave's weight fragments: channel tile cout0 / 16 + wave, [k32 step][plane][lane]
    const char* wsrc = (const char*)a.w + (size_t)(cout0 / 16 + wave) * (a.cin / 32) * 16 * 1024 + lane * 16;
    f32x4 acc[16][2];
#pragma unroll
    for (int p = 0; p < 16; ++p)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[p][j] = f32x4{0, 0, 0, 0};
#pragma unroll 1
    for (int ks = 0; ks < nks; ++ks) {
      if constexpr (PRE) {
        const int c = (ks * 8 + g) * 8;
        const f32x4 sc0 = *(const f32x4*)(a.scale_in + c), sc1 = *(const f32x4*)(a.scale_in + c + 4);
        const f32x4 sh0 = *(const f32x4*)(a.shift_in + c), sh1 = *(const f32x4*)(a.shift_in + c + 4);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (!(onboard >> i & 1)) continue;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            d[i][e] = (_Float16)mish_f(__builtin_fmaf((float)d[i][e], sc0[e], sh0[e]));
            d[i][4 + e] = (_Float16)mish_f(__builtin_fmaf((float)d[i][4 + e], sc1[e], sh1[e]));
          }
        }
      }
      // V = B^T d B, B^T = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]: first down the rows, then along them
      h8 t[16];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        t[c] = d[c] - d[8 + c];
        t[4 + c] = d[4 + c] + d[8 + c];
        t[8 + c] = d[8 + c] - d[4 + c];
        t[12 + c] = d[4 + c] - d[12 + c];
      }
      char* vdst = smem + g * (kWinoUnitTiles * 16) + ts * 16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        *(h8*)(vdst + (4 * r + 0) * kVPlane) = t[4 * r] - t[4 * r + 2];
        *(h8*)(vdst + (4 * r + 1) * kVPlane) = t[4 * r + 1] + t[4 * r + 2];
        *(h8*)(vdst + (4 * r + 2) * kVPlane) = t[4 * r + 2] - t[4 * r + 1];
        *(h8*)(vdst + (4 * r + 3) * kVPlane) = t[4 * r + 1] - t[4 * r + 3];
      }
      // (pinned: hoisted above the transform, the fragment loads cost it its registers)
      __builtin_amdgcn_sched_barrier(0);
      h8 af[2][16];
#pragma unroll
      for (int p = 0; p < 16; ++p) af[0][p] = *(const h8*)(wsrc + ((size_t)ks * 32 + p) * 1024);
      if (ks + 1 < nks) patch_load(ks + 1);
      __syncthreads();
#pragma unroll
      for (int p = 0; p < 16; ++p) af[1][p] = *(const h8*)(wsrc + ((size_t)ks * 32 + 16 + p) * 1024);
      // the two k32 steps of the slice, plane by plane
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const char* vsrc = smem + (4 * sub + q) * (kWinoUnitTiles * 16) + (lane & 15) * 16;
#pragma unroll
        for (int p = 0; p < 16; ++p)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const h8 b = *(const h8*)(vsrc + p * kVPlane + j * 256);
            acc[p][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[sub][p], b, acc[p][j], 0, 0, 0);
          }
      }
      __syncthreads();   // the next slice, or the next unit, rewrites V
    }
    // ---- Y = A^T M A, A^T = [[1, 1, 1, 0], [0, 1, -1, -1]], in fp32: down the rows first, left to right; then the epilogue
    const int c = cout0 + wave * 16 + 4 * q;   // the lane's four output channels
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int tl = 16 * j + (lane & 15);
      if (tl >= ntiles) continue;
      const long of = tile0 + tl;
      const int opos = (int)(of / kWinoTiles), ot = (int)(of - (long)opos * kWinoTiles);
      const int oy = 2 * (ot / 10), ox = 2 * (ot % 10);
      f32x4 s0[4], s1[4];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        s0[cc] = (acc[cc][j] + acc[4 + cc][j]) + acc[8 + cc][j];
        s1[cc] = (acc[4 + cc][j] - acc[8 + cc][j]) - acc[12 + cc][j];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const f32x4* s = i ? s1 : s0;
          f32x4 v = k ? (s[1] - s[2]) - s[3] : (s[0] + s[1]) + s[2];
          if (oy + i >= kBL || ox + k >= kBL) continue;
          const int loc = (oy + i) * kBL + ox + k;
          const size_t o = ((size_t)opos * (a.cout / 8) + (c >> 3)) * kPosHalves + loc * 8 + (c & 7);
          if (a.res) {
            const h4 r = *(const h4*)(a.out + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += (float)r[e];
          }
          if (a.dual) *(h4*)(a.out + o) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
          if (a.act == 1 || a.dual) {
            const f32x4 sc = *(const f32x4*)(a.scale_out + c), sh = *(const f32x4*)(a.shift_out + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = mish_f(__builtin_fmaf(v[e], sc[e], sh[e]));
          }
          *(h4*)((a.dual ? a.out2 : a.out) + o) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        }
    }
  }
}

// =======================================================================================
// Host-side launcher
// =======================================================================================
hipError_t launch_wconv(const WConvArgs& a, int n_cu, hipStream_t s) {
  auto width_ok = [](int c) { return c >= 64 && c <= kWinoMaxC && c % 64 == 0; };
  if (!width_ok(a.cin) || !width_ok(a.cout) || a.npos < 1 || n_cu < 1) return hipErrorInvalidValue;
  if (a.act < 0 || a.act > 1 || (a.act && a.dual) || (a.dual && !a.out2)) return hipErrorInvalidValue;
  const dim3 grid(wconv_grid(a.npos, a.cout, n_cu));
  if (a.pre) hipLaunchKernelGGL(k_wconv<true>, grid, dim3(kWWG), 0, s, a);
  else hipLaunchKernelGGL(k_wconv<false>, grid, dim3(kWWG), 0, s, a);
  return hipGetLastError();
}

const char* wconv_kernel_name() { return "k_wconv"; }

}  // namespace p3
