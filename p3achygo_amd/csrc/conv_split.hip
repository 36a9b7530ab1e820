// conv_split.hip — k_sconv<KW>, the layer conv of the low-latency plan (conv_split.h, P3HIP_FLAG_LOW_LATENCY), for gfx950.
//
// Per item (position, T output channels, strip of board rows) the conv is a GEMM out[cout][point] = sum over
// (cin, tap) W[tap][cin][cout] * in[cin][point + tap] on v_mfma_f32_16x16x32_f16: the weights are the A operand (16
// output channels x 32 input channels), the activations the B operand (32 input channels x 16 board points: lane
// quarter q holds the 16-byte piece of channel group q), and a lane's four accumulators are four consecutive output
// channels of one board point, half a piece of the output.  The four waves of a workgroup share the item's T / 16
// channel tiles and take every fourth tile of 16 points; a point's tile is counted along the strip's own points
// (19 per row), so 361 / 190 / 95 points are 23 / 12 / 6 tiles whatever the kernel size.
//
// K runs in slices of 32 channels (3x3: one MFMA step per tap) or 64 (1x1: two steps), slice by slice, step by step, tap
// by tap: one chain per output, the same for every split.  LDS holds one slice of the strip as planes of 8 channels,
// [group][slot][8], slot = PAD + row * (19 + PAD) + x over the strip's rows and its halo rows: the pad slot between two
// rows serves both, pad slots are zeroed once and never written, halo rows outside the board are written as zeros.  A
// plane is a multiple of 16 slots, which keeps the four lane quarters of a ds_read_b128 group on different banks.  Behind
// the planes lie the slice's weight fragments of the item's tile, copied as they are packed (pack_sconv): 1 KB each,
// read back by lane.  The next slice's activations and fragments are fetched into registers while the MFMAs of the
// current one run.
// Activation offsets are 64-bit per position; the 32-bit offsets stay inside one position's C x 361 halves.
#include "conv_split.h"

#include <hip/hip_runtime.h>

#include "conv_core.h"   // mish_f, h8, h4, f32x4

namespace p3 {

namespace {

constexpr int kSWG = 256;
constexpr int kPosHalves = kNLoc * 8;   // one channel group of one position
constexpr int kMaxMT = 4, kMaxNT = 6;   // channel tiles of an item, point tiles of a wave (23 tiles over 4 waves)

template <int KW>
struct GeoS {
  static constexpr int PAD = KW / 2, RS = kBL + PAD, TAPS = KW * KW;
  static constexpr int KSTEPS = KW == 3 ? 1 : 2;   // MFMA k steps (32 channels) per slice
  static constexpr int NG = 4 * KSTEPS;            // channel groups per slice
  static constexpr int MAXROWS = kBL + 2 * PAD;
  static constexpr int NSLOT = (PAD + MAXROWS * RS + PAD + 15) / 16 * 16;
  static constexpr int PLANE = NSLOT * 16;         // bytes
  static constexpr int ACT_BYTES = NG * PLANE;
  static constexpr int WFRAGS = KSTEPS * TAPS;     // fragments of one channel tile and slice
  static constexpr int W_BYTES = kMaxMT * WFRAGS * 1024;
  static constexpr int XP = (NG * MAXROWS * kBL + kSWG - 1) / kSWG;   // activation pieces per thread and slice
  static constexpr int WP = kMaxMT * WFRAGS * 64 / kSWG;              // weight pieces
};

// the geometry of one item
struct Item {
  int pos, ct0, r0, nrows;   // first channel tile (of 16), first board row, rows
};

// the slice's pieces -> registers
template <int KW>
__device__ __forceinline__ void slice_load(const SConvArgs& a, const Item& it, int nmt, int sl, h8 (&xr)[GeoS<KW>::XP],
                                           h8 (&wr)[GeoS<KW>::WP]) {
  using G = GeoS<KW>;
  const _Float16* src = a.in + (size_t)it.pos * a.cin * kNLoc + (size_t)sl * G::NG * kPosHalves;
  const int nst = (it.nrows + 2 * G::PAD) * kBL;   // staged points
#pragma unroll
  for (int i = 0; i < G::XP; ++i) {
    const int idx = threadIdx.x + kSWG * i, g = idx % G::NG, rem = idx / G::NG;
    const int ly = rem / kBL, x = rem - ly * kBL, y = it.r0 - G::PAD + ly;
    xr[i] = h8{0, 0, 0, 0, 0, 0, 0, 0};
    if (rem < nst && y >= 0 && y < kBL) xr[i] = *(const h8*)(src + g * kPosHalves + (y * kBL + x) * 8);
  }
  const char* wsrc = (const char*)a.w + ((size_t)it.ct0 * (a.cin / 32) + (size_t)sl * G::KSTEPS) * G::TAPS * 1024;
  const size_t ct_stride = (size_t)(a.cin / 32) * G::TAPS * 1024;
#pragma unroll
  for (int i = 0; i < G::WP; ++i) {
    const int idx = threadIdx.x + kSWG * i, ctl = idx / (G::WFRAGS * 64), within = idx - ctl * (G::WFRAGS * 64);
    if (ctl < nmt) wr[i] = *(const h8*)(wsrc + ctl * ct_stride + within * 16);
  }
}

// registers -> LDS, the activations through mish(bn_in(.)) when pre
template <int KW>
__device__ __forceinline__ void slice_store(const SConvArgs& a, const Item& it, int nmt, int sl, char* smem,
                                            const h8 (&xr)[GeoS<KW>::XP], const h8 (&wr)[GeoS<KW>::WP]) {
  using G = GeoS<KW>;
  const int nst = (it.nrows + 2 * G::PAD) * kBL;
#pragma unroll
  for (int i = 0; i < G::XP; ++i) {
    const int idx = threadIdx.x + kSWG * i, g = idx % G::NG, rem = idx / G::NG;
    if (rem >= nst) continue;
    const int ly = rem / kBL, x = rem - ly * kBL, y = it.r0 - G::PAD + ly;
    h8 v = xr[i];
    if (a.pre && y >= 0 && y < kBL) {
      const int c = (sl * G::NG + g) * 8;
      const f32x4 sc0 = *(const f32x4*)(a.scale_in + c), sc1 = *(const f32x4*)(a.scale_in + c + 4);
      const f32x4 sh0 = *(const f32x4*)(a.shift_in + c), sh1 = *(const f32x4*)(a.shift_in + c + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = (_Float16)mish_f(__builtin_fmaf((float)v[e], sc0[e], sh0[e]));
        v[4 + e] = (_Float16)mish_f(__builtin_fmaf((float)v[4 + e], sc1[e], sh1[e]));
      }
    }
    *(h8*)(smem + g * G::PLANE + (G::PAD + ly * G::RS + x) * 16) = v;
  }
#pragma unroll
  for (int i = 0; i < G::WP; ++i) {
    const int idx = threadIdx.x + kSWG * i;
    if (idx / (G::WFRAGS * 64) < nmt) *(h8*)(smem + G::ACT_BYTES + idx * 16) = wr[i];
  }
}

// the MFMAs of one slice: MT channel tiles x the wave's nj point tiles, step by step, tap by tap
template <int KW, int MT>
__device__ __forceinline__ void slice_mma(const char* smem, const int (&base)[kMaxNT], int nj, f32x4 (&acc)[kMaxMT][kMaxNT]) {
  using G = GeoS<KW>;
  const char* wl = smem + G::ACT_BYTES + (threadIdx.x & 63) * 16;
#pragma unroll
  for (int ks = 0; ks < G::KSTEPS; ++ks)
#pragma unroll
    for (int tap = 0; tap < G::TAPS; ++tap) {
      h8 af[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) af[mt] = *(const h8*)(wl + ((mt * G::KSTEPS + ks) * G::TAPS + tap) * 1024);
      const int toff = ks * 4 * G::PLANE + ((tap / KW) * G::RS + tap % KW) * 16;
#pragma unroll
      for (int j = 0; j < kMaxNT; ++j) {
        if (j >= nj) break;
        const h8 b = *(const h8*)(smem + base[j] + toff);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], b, acc[mt][j], 0, 0, 0);
      }
    }
}

}  // namespace

template <int KW>
__global__ void __launch_bounds__(kSWG) k_sconv(SConvArgs a) {
  using G = GeoS<KW>;
  __shared__ __attribute__((aligned(16))) char smem[G::ACT_BYTES + G::W_BYTES];
  for (int i = threadIdx.x * 16; i < G::ACT_BYTES; i += kSWG * 16) *(f32x4*)(smem + i) = f32x4{0, 0, 0, 0};
  __syncthreads();
  const int S = a.strips, nmt = a.tile / 16, ntile = a.cout / a.tile, nsl = a.cin / (32 * G::KSTEPS);
  const int rows_per = (kBL + S - 1) / S;
  const long items = (long)a.npos * ntile * S;
  const int lane = threadIdx.x & 63, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    Item it;
    const int strip = (int)(item % S);
    const long pt = item / S;
    it.pos = (int)(pt / ntile);
    it.ct0 = (int)(pt - (long)it.pos * ntile) * nmt;
    it.r0 = strip * rows_per;
    it.nrows = (it.r0 + rows_per < kBL ? it.r0 + rows_per : kBL) - it.r0;
    const int npts = it.nrows * kBL;
    const int nj = __builtin_amdgcn_readfirstlane(((npts + 15) / 16 - wave + 3) / 4);
    // the LDS byte offset of this lane's point in each of the wave's point tiles (tap (0, 0), plane of group q); lanes
    // beyond the strip's last point read that point again and store nothing
    int base[kMaxNT];
#pragma unroll
    for (int j = 0; j < kMaxNT; ++j) {
      int p = (wave + 4 * j) * 16 + (lane & 15);
      p = p < npts ? p : npts - 1;
      const int orow = p / kBL;
      base[j] = q * G::PLANE + (orow * G::RS + (p - orow * kBL)) * 16;
    }
    f32x4 acc[kMaxMT][kMaxNT];
#pragma unroll
    for (int mt = 0; mt < kMaxMT; ++mt)
#pragma unroll
      for (int j = 0; j < kMaxNT; ++j) acc[mt][j] = f32x4{0, 0, 0, 0};
    h8 xr[G::XP], wr[G::WP];
    slice_load<KW>(a, it, nmt, 0, xr, wr);
#pragma unroll 1
    for (int sl = 0; sl < nsl; ++sl) {
      slice_store<KW>(a, it, nmt, sl, smem, xr, wr);
      __syncthreads();
      if (sl + 1 < nsl) slice_load<KW>(a, it, nmt, sl + 1, xr, wr);
      if (nmt == 4) slice_mma<KW, 4>(smem, base, nj, acc);
      else if (nmt == 2) slice_mma<KW, 2>(smem, base, nj, acc);
      else slice_mma<KW, 1>(smem, base, nj, acc);
      __syncthreads();   // the next slice, or the next item, rewrites the planes and the fragments
    }
    // epilogue: four output channels of one point per accumulator
#pragma unroll
    for (int j = 0; j < kMaxNT; ++j) {
      if (j >= nj) break;
      const int p = (wave + 4 * j) * 16 + (lane & 15);
      if (p >= npts) continue;
      const int loc = it.r0 * kBL + p;
#pragma unroll
      for (int mt = 0; mt < kMaxMT; ++mt) {
        if (mt >= nmt) break;
        const int c = (it.ct0 + mt) * 16 + 4 * q;
        const size_t o = ((size_t)it.pos * (a.cout / 8) + (c >> 3)) * kPosHalves + loc * 8 + (c & 7);
        f32x4 v = acc[mt][j];
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
        } else if (a.act == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = mish_f(v[e]);
        }
        *(h4*)((a.dual ? a.out2 : a.out) + o) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
      }
    }
  }
}

// =======================================================================================
// Host-side launcher
// =======================================================================================
namespace {
bool width_ok(int c) { return c >= 64 && c <= kSplitMaxC && c % 64 == 0; }
}  // namespace

hipError_t launch_sconv(int kw, const SConvArgs& a, int n_cu, hipStream_t s) {
  if (!width_ok(a.cin) || !width_ok(a.cout) || a.npos < 1 || (kw != 1 && kw != 3) || !sconv_split_valid(a.strips, a.tile))
    return hipErrorInvalidValue;
  if ((a.act != 0 && a.dual) || a.act < 0 || a.act > 2) return hipErrorInvalidValue;
  // one workgroup per CU (the kernel's registers allow one wave per SIMD), the items dealt round
  const long items = (long)a.npos * a.strips * (a.cout / a.tile);
  const int grid = (int)(items < (long)n_cu ? items : (long)n_cu);
  if (kw == 3) hipLaunchKernelGGL(k_sconv<3>, dim3(grid), dim3(kSWG), 0, s, a);
  else hipLaunchKernelGGL(k_sconv<1>, dim3(grid), dim3(kSWG), 0, s, a);
  return hipGetLastError();
}

const char* sconv_kernel_name(int kw) { return kw == 3 ? "k_sconv<3>" : "k_sconv<1>"; }

}  // namespace p3
